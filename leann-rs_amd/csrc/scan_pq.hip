// scan_pq.hip — PQ rows: one byte per dsub (4 or 8) columns, the index of the nearest of 256 trained centroids, searched exhaustively by
// an asymmetric-distance scan over per-query lookup tables held in LDS (include/leann_backend.h "PQ rows"):
// leann_pq_rows_*, leann_pq_train[_device], leann_pq_encode, leann_pq_query_lut and the two search calls with their host-pointer twins.
//
// A row is M = ceil(dims / dsub) code bytes, padded with zero bytes to MP = 16 ceil(M / 16); a query is M tables of 256 int16 entries
// w[m][c] (its inner product with centroid c of sub-space m under one power-of-two scale per query), the score t_i = sum_m
// w[m][code[i][m]] in int32; the fetch_k best rows by t_i are the answer, the refined call hands them to leann_rerank_batch_device.
// This is the one scan of the tree whose inner loop is no matrix instruction: it is a gather from LDS.
//
// Kernels:
//   pq_encode_kernel<DSUB>   a workgroup owns 256 consecutive rows, thread t row t, and takes one sub-space at a time: its 256 x DSUB
//                            centroids go into LDS (8 KiB at DSUB = 8), the lane keeps its row's sub-vector in registers and walks the
//                            centroids by broadcast reads (every lane the same address), keeping the minimum of the difference-form
//                            distance (pq_dist, which the host reference compiles too) under a strict <: no cross-lane step, ties to the
//                            lower c.  The 8 codes of a slice leave as one 8-B store into the object's layout.  The trainer's
//                            assignment step is this kernel.
//   pq_lut_kernel<DSUB>      one workgroup per query, thread c the centroid c of every sub-space: float64 chains (pq_dot) twice — first
//                            for max |L| and finiteness, then for the int16 entries —, one "no tables" word per query.
//   score_pq_kernel<LIST>    the hot path, below.
//   pq_no_answer_kernel      keys, scores and count of a query without tables (or of every query when no row is allowed): all tail.
//   pq_init_centroids_kernel, pq_update_kernel<DSUB>   the trainer: centroid c starts as row floor(c n / 256); an update is one thread
//                            per (centroid, column) walking the assignments in sample order with a float64 sum, so the result is
//                            the same bytes on every run (no atomic sum anywhere).
//
// score_pq_kernel.  Tables are query-interleaved: for a group of BQ = 8 queries the entry of (m, c) is 8 consecutive int16, 16 B, so one
// ds_read_b128 at an address made from a row's code byte serves eight (row, query) pairs.  A slice is MS = 8 sub-spaces: 8 x 256 x 16 B
// = 32 KiB of tables, two buffers of it (64 KiB static LDS, the whole static limit, two workgroups per CU): while slice s is gathered,
// slice s + 1 travels through registers (8 global b128 loads per thread, contiguous: the table array is laid out [group][m][c][8]) and
// is written to the other buffer behind the gather; one __syncthreads per slice.  A thread owns RPT = 8 rows x 8 queries = 64 int32
// accumulators, a workgroup 2 048 rows, so the table bytes staged per tile (32 KiB per slice) are a sixteenth of the bytes gathered
// from them (2 048 rows x 8 x 16 B).  Lane l of pass r owns row 256 r + tid: the slab stores of a wave are whole 256-B lines.
//
// Row layout on the device: rows in blocks of 64; the 8 code bytes of (row, slice) for the 64 rows of a block are one contiguous 512-B
// run, block-major, then slice: byte ((row / 64) NS + s) 512 + (row % 64) 8 + m % 8, NS = MP / 8 slices.  A wave's code load for a
// slice is one 8-B word per lane, 512 contiguous bytes.  leann_pq_rows_export undoes the layout on the host.
//
// Accumulation: every 16-bit entry goes into a 32-bit accumulator (|t| reaches 2^24); see PQ_ACC below for the form chosen from the ISA.
//
// Banks (reasoned, not counted): a ds_read_b128 of a wave is served in four groups of 16 lanes, each group's 16 x 16 B filling the 64
// banks once when the 16 slots differ modulo 16 (a sub-space's 256 slots of 16 B are 16 rows of the 64-bank array).  For 16 random
// codes the expected largest number of lanes on one of the 16 bank groups is about 3 (balls in bins, 16 into 16), so a gather runs
// at roughly a third of the conflict-free LDS rate on random codes; lanes that hold the same code read the same address and are
// served together.
#include "common.cuh"
#include "../../include/leann_backend.h"
#include "search.cuh"
#include "internal.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef short i16x2 __attribute__((ext_vector_type(2)));
// Queries of a table group, sub-spaces of a slice, rows per thread.  The resource report (hipcc -Rpass-analysis=kernel-resource-usage,
// gfx950; nothing spills, no scratch): see DESIGN.md §9k for the table and the alternatives that were compiled.
constexpr uint32_t PQ_BQ = 8, PQ_MS = 8, PQ_RPT = 8, PQ_BR = 256 * PQ_RPT;
constexpr uint32_t PQ_ET = 256; // rows of an encode tile
constexpr size_t PQ_MAX_K = SEG / 2, PQ_MAX_DIMS = 4096;

struct PqShape {
    size_t dims, dsub, M, MP, NS; // sub-spaces, the row pitch MP = 16 ceil(M / 16), slices of 8 sub-spaces
};
static inline PqShape pq_shape(size_t dims, size_t dsub) {
    const size_t M = (dims + dsub - 1) / dsub, MP = (M + 15) / 16 * 16;
    return {dims, dsub, M, MP, MP / PQ_MS};
}
static inline size_t pq_rows64(size_t n) { return (n + 63) / 64 * 64; }
static inline size_t pq_query_rows(size_t nq) { return (nq + PQ_BQ - 1) / PQ_BQ * PQ_BQ; }
// byte of (row, sub-space m) in the device layout
static inline size_t pq_code_at(size_t row, size_t m, size_t NS) { return ((row >> 6) * NS + (m >> 3)) * 512 + (row & 63) * 8 + (m & 7); }

// ---- the definition, steps 1 and 2: host and device compile the same functions ------------------------------------------------------
#define PQ_FN __host__ __device__ __forceinline__
PQ_FN bool pq_finite(float x) { return (__builtin_bit_cast(uint32_t, x) & 0x7FFFFFFFu) < 0x7F800000u; }
PQ_FN float pq_clean(float x) { return pq_finite(x) ? x : 0.f; } // an element that is not finite counts as 0
// sum_j (x_j - c_j)^2 in f32, the difference form (built without contraction, so host and device give the same bits)
template <int DSUB>
PQ_FN float pq_dist(const float *x, const float *c) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < DSUB; j++) {
        const float d = x[j] - c[j];
        s = s + d * d;
    }
    return s;
}
// sum_j q_j c_j in float64, j ascending; every product is exact, the caller rounds the sum once to f32
template <int DSUB>
PQ_FN double pq_dot(const float *q, const float *c) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < DSUB; j++) s = s + (double)q[j] * (double)c[j];
    return s;
}
// w = rne(L 2^(140 - E)): the power of two is built from its bits, the product is exact in float64
PQ_FN int pq_entry(float L, uint32_t E) {
    const double scale = __builtin_bit_cast(double, (uint64_t)(1023u + 140u - E) << 52);
    return (int)rint((double)L * scale);
}

// ---- the row codes -------------------------------------------------------------------------------------------------------------------
// X [n x ld] f32 -> codes in the device layout, from the block of the launch's first row on (that row is a multiple of 64 in the
// object); rows n .. n_pad - 1 (n_pad = n rounded up to 64) get zero bytes.  C [M][256][DSUB], padding columns zero.
template <int DSUB>
__global__ void __launch_bounds__(256) pq_encode_kernel(const float *__restrict__ X, uint64_t n, uint64_t n_pad, uint32_t d, uint64_t ld,
                                                        const float *__restrict__ C, uint32_t M, uint32_t NS, uint8_t *__restrict__ codes) {
    __shared__ float sC[256 * DSUB];
    const uint32_t tid = threadIdx.x;
    const uint64_t row = (uint64_t)blockIdx.x * PQ_ET + tid;
    const bool live = row < n;
    const float *x = X + (live ? row : n - 1) * ld;
    for (uint32_t s = 0; s < NS; s++) {
        uint32_t w[2] = {0u, 0u};
#pragma unroll
        for (uint32_t mm = 0; mm < PQ_MS; mm++) {
            const uint32_t m = s * PQ_MS + mm;
            if (m >= M) break; // the same for the whole workgroup
            __syncthreads(); // the walk of the sub-space before is over
#pragma unroll
            for (int j = 0; j < DSUB; j += 4)
                *reinterpret_cast<float4 *>(sC + tid * DSUB + j) = *reinterpret_cast<const float4 *>(C + ((size_t)m * 256 + tid) * DSUB + j);
            float xv[DSUB];
#pragma unroll
            for (int j = 0; j < DSUB; j++) {
                const uint32_t col = m * DSUB + j;
                xv[j] = live && col < d ? pq_clean(x[col]) : 0.f;
            }
            __syncthreads();
            float best = pq_dist<DSUB>(xv, sC);
            uint32_t bi = 0;
            for (uint32_t c = 1; c < 256; c++) {
                const float dd = pq_dist<DSUB>(xv, sC + c * DSUB);
                if (dd < best) { best = dd; bi = c; }
            }
            w[mm >> 2] |= bi << (8 * (mm & 3));
        }
        if (row < n_pad)
            *reinterpret_cast<uint2 *>(codes + (((row >> 6) * NS + s) * 64 + (row & 63)) * 8) = live ? make_uint2(w[0], w[1]) : make_uint2(0u, 0u);
    }
}

static int pq_check_shape(const char *who, size_t dims, size_t dsub) {
    if (dims < 1 || dims > PQ_MAX_DIMS) { leann_set_error("%s: dims = %zu is outside [1, 4096]", who, dims); return LEANN_ERR_INVALID; }
    if (dsub != 4 && dsub != 8) { leann_set_error("%s: dsub = %zu is neither 4 nor 8", who, dsub); return LEANN_ERR_INVALID; }
    return LEANN_OK;
}
// caller's codebooks [M][256][dsub] -> the same with every column at or behind dims zero; refuses a value that is not finite
static int pq_take_codebooks(const char *who, const float *codebooks, const PqShape &sh, std::vector<float> *out) {
    if (!codebooks) { leann_set_error("%s: null codebooks", who); return LEANN_ERR_INVALID; }
    out->assign(sh.M * 256 * sh.dsub, 0.f);
    for (size_t m = 0; m < sh.M; m++)
        for (size_t c = 0; c < 256; c++)
            for (size_t j = 0; j < sh.dsub && m * sh.dsub + j < sh.dims; j++) {
                const float v = codebooks[(m * 256 + c) * sh.dsub + j];
                if (!pq_finite(v)) {
                    leann_set_error("%s: codebooks hold a value that is not finite (sub-space %zu, centroid %zu)", who, m, c);
                    return LEANN_ERR_INVALID;
                }
                (*out)[(m * 256 + c) * sh.dsub + j] = v;
            }
    return LEANN_OK;
}

template <int DSUB>
static void pq_encode_host(const float *rows, size_t n, const PqShape &sh, const float *cb, uint8_t *out) {
    for (size_t i = 0; i < n; i++)
        for (size_t m = 0; m < sh.M; m++) {
            float xv[DSUB];
            for (size_t j = 0; j < DSUB; j++) xv[j] = m * DSUB + j < sh.dims ? pq_clean(rows[i * sh.dims + m * DSUB + j]) : 0.f;
            float best = pq_dist<DSUB>(xv, cb + m * 256 * DSUB);
            uint32_t bi = 0;
            for (uint32_t c = 1; c < 256; c++) {
                const float dd = pq_dist<DSUB>(xv, cb + (m * 256 + c) * DSUB);
                if (dd < best) { best = dd; bi = c; }
            }
            out[i * sh.MP + m] = (uint8_t)bi;
        }
}

extern "C" int leann_pq_encode(const float *rows, size_t n, size_t dims, size_t dsub, const float *codebooks, uint8_t *out) {
    const char *who = "leann_pq_encode";
    if (int rc = pq_check_shape(who, dims, dsub)) return rc;
    if ((!rows || !out) && n) { leann_set_error("%s: null %s", who, !rows ? "rows" : "out"); return LEANN_ERR_INVALID; }
    const PqShape sh = pq_shape(dims, dsub);
    std::vector<float> cb;
    if (int rc = pq_take_codebooks(who, codebooks, sh, &cb)) return rc;
    if (n) memset(out, 0, n * sh.MP);
    if (dsub == 4) pq_encode_host<4>(rows, n, sh, cb.data(), out);
    else pq_encode_host<8>(rows, n, sh, cb.data(), out);
    return LEANN_OK;
}

template <int DSUB>
static int pq_lut_host(const float *q, const PqShape &sh, const float *cb, int16_t *out) {
    std::vector<float> qp(sh.M * DSUB, 0.f), L(sh.M * 256);
    bool ok = true;
    for (size_t j = 0; j < sh.dims; j++) ok &= pq_finite(qp[j] = q[j]);
    uint32_t mb = 0;
    for (size_t m = 0; m < sh.M && ok; m++)
        for (size_t c = 0; c < 256; c++) {
            L[m * 256 + c] = (float)pq_dot<DSUB>(qp.data() + m * DSUB, cb + (m * 256 + c) * DSUB);
            mb = std::max(mb, __builtin_bit_cast(uint32_t, L[m * 256 + c]) & 0x7FFFFFFFu);
        }
    if (!ok || mb >= 0x7F800000u) return 1;
    const uint32_t E = std::max(mb >> 23, 1u);
    for (size_t i = 0; i < sh.M * 256; i++) out[i] = (int16_t)pq_entry(L[i], E);
    return 0;
}

extern "C" int leann_pq_query_lut(const float *q, size_t dims, size_t dsub, const float *codebooks, int16_t *out) {
    const char *who = "leann_pq_query_lut";
    if (int rc = pq_check_shape(who, dims, dsub)) return rc;
    if (!q || !out) { leann_set_error("%s: null %s", who, !q ? "q" : "out"); return LEANN_ERR_INVALID; }
    const PqShape sh = pq_shape(dims, dsub);
    std::vector<float> cb;
    if (int rc = pq_take_codebooks(who, codebooks, sh, &cb)) return rc;
    memset(out, 0, sh.M * 256 * sizeof(int16_t));
    if (dsub == 4 ? pq_lut_host<4>(q, sh, cb.data(), out) : pq_lut_host<8>(q, sh, cb.data(), out)) {
        leann_set_error("%s: the query has no tables (an element or a table entry is not finite)", who);
        return 1;
    }
    return LEANN_OK;
}

// ---- the object ------------------------------------------------------------------------------------------------------------------------
struct leann_pq_rows {
    size_t n = 0;
    PqShape sh{};
    int device = 0;
    uint64_t key_offset = 0;
    std::vector<float> cb_host; // [M][256][dsub], padding columns zero
    DeviceBuf<float> cb;        // the same on the device
    DeviceBuf<uint8_t> codes;   // [n rounded up to 64 x MP] in the block layout of the file header
};

static void pq_launch_encode(const float *d_rows, size_t rows, const PqShape &sh, size_t ld, const float *d_cb, uint8_t *codes) {
    const dim3 grid((unsigned)((pq_rows64(rows) + PQ_ET - 1) / PQ_ET));
    if (sh.dsub == 4)
        hipLaunchKernelGGL(pq_encode_kernel<4>, grid, dim3(256), 0, nullptr, d_rows, (uint64_t)rows, (uint64_t)pq_rows64(rows), (uint32_t)sh.dims,
                           (uint64_t)ld, d_cb, (uint32_t)sh.M, (uint32_t)sh.NS, codes);
    else
        hipLaunchKernelGGL(pq_encode_kernel<8>, grid, dim3(256), 0, nullptr, d_rows, (uint64_t)rows, (uint64_t)pq_rows64(rows), (uint32_t)sh.dims,
                           (uint64_t)ld, d_cb, (uint32_t)sh.M, (uint32_t)sh.NS, codes);
}

static int pq_new_check(const char *who, size_t n, size_t dims, size_t dsub, int device, const void *out) {
    if (!out) { leann_set_error("%s: null out", who); return LEANN_ERR_INVALID; }
    if (int rc = pq_check_shape(who, dims, dsub)) return rc;
    if (n >= 0xFFFFFFFFull) { leann_set_error("%s: n = %zu is 2^32 - 1 or more", who, n); return LEANN_ERR_INVALID; }
    if (device < 0) { leann_set_error("%s: device = %d", who, device); return LEANN_ERR_INVALID; }
    return LEANN_OK;
}
static int pq_new(const char *who, size_t n, size_t dims, size_t dsub, const float *codebooks, int device, uint64_t key_offset,
                  std::unique_ptr<leann_pq_rows> *out) {
    std::unique_ptr<leann_pq_rows> b(new leann_pq_rows());
    b->n = n; b->sh = pq_shape(dims, dsub); b->device = device; b->key_offset = key_offset;
    if (int rc = pq_take_codebooks(who, codebooks, b->sh, &b->cb_host)) return rc;
    if (int rc = leann_internal_check_device(device)) return rc;
    HIP_CHECK_RET(hipSetDevice(device));
    if (int rc = b->cb.alloc(b->cb_host.size())) return rc;
    HIP_CHECK_RET(hipMemcpy(b->cb, b->cb_host.data(), b->cb_host.size() * 4, hipMemcpyHostToDevice));
    if (int rc = b->codes.alloc(pq_rows64(n) * b->sh.MP)) return rc;
    *out = std::move(b);
    return LEANN_OK;
}
// rows [rows x ld] on the device -> the codes of positions row0 .. (row0 a multiple of 64)
static int pq_encode_rows(leann_pq_rows *b, const float *d_rows, size_t row0, size_t rows, size_t ld) {
    if (rows == 0) return LEANN_OK;
    pq_launch_encode(d_rows, rows, b->sh, ld, b->cb, b->codes.p + row0 * b->sh.MP);
    HIP_CHECK_RET(hipGetLastError());
    HIP_CHECK_RET(hipStreamSynchronize(nullptr)); // the source rows are the caller's (or a slab that is filled again next)
    return LEANN_OK;
}

extern "C" int leann_pq_rows_from_device(const float *d_rows, size_t n, size_t dims, size_t ld, const float *codebooks, size_t dsub, int device,
                                         uint64_t key_offset, leann_pq_rows **out) {
    const char *who = "leann_pq_rows_from_device";
    if (out) *out = nullptr;
    if (int rc = pq_new_check(who, n, dims, dsub, device, out)) return rc;
    if (!d_rows && n) { leann_set_error("%s: null d_rows", who); return LEANN_ERR_INVALID; }
    if (ld < dims) { leann_set_error("%s: ld = %zu is below dims = %zu", who, ld, dims); return LEANN_ERR_INVALID; }
    std::unique_ptr<leann_pq_rows> b;
    if (int rc = pq_new(who, n, dims, dsub, codebooks, device, key_offset, &b)) return rc;
    if (int rc = pq_encode_rows(b.get(), d_rows, 0, n, ld)) return rc;
    *out = b.release();
    return LEANN_OK;
}

extern "C" int leann_pq_rows_from_host(const float *rows, size_t n, size_t dims, const float *codebooks, size_t dsub, int device,
                                       uint64_t key_offset, leann_pq_rows **out) {
    const char *who = "leann_pq_rows_from_host";
    if (out) *out = nullptr;
    if (int rc = pq_new_check(who, n, dims, dsub, device, out)) return rc;
    if (!rows && n) { leann_set_error("%s: null rows", who); return LEANN_ERR_INVALID; }
    std::unique_ptr<leann_pq_rows> b;
    if (int rc = pq_new(who, n, dims, dsub, codebooks, device, key_offset, &b)) return rc;
    // slabs of at most 256 MiB of f32 rows, whole encode tiles each: the collection itself never has to fit beside its codes
    const size_t slab_rows = std::min<size_t>(pq_rows64(n), std::max<size_t>(PQ_ET, ((size_t)256 << 20) / (dims * 4) / PQ_ET * PQ_ET));
    DeviceBuf<float> slab;
    if (n)
        if (int rc = slab.alloc(slab_rows * dims)) return rc;
    for (size_t r0 = 0; r0 < n; r0 += slab_rows) {
        const size_t m = std::min(slab_rows, n - r0);
        HIP_CHECK_RET(hipMemcpy(slab, rows + r0 * dims, m * dims * 4, hipMemcpyHostToDevice));
        if (int rc = pq_encode_rows(b.get(), slab, r0, m, dims)) return rc;
    }
    *out = b.release();
    return LEANN_OK;
}

extern "C" size_t leann_pq_rows_len(const leann_pq_rows *b) { return b ? b->n : 0; }
extern "C" size_t leann_pq_rows_dims(const leann_pq_rows *b) { return b ? b->sh.dims : 0; }
extern "C" size_t leann_pq_rows_dsub(const leann_pq_rows *b) { return b ? b->sh.dsub : 0; }
extern "C" size_t leann_pq_rows_pitch(const leann_pq_rows *b) { return b ? b->sh.MP : 0; }
extern "C" int leann_pq_rows_codebooks(const leann_pq_rows *b, float *out) {
    if (!b || !out) { leann_set_error("leann_pq_rows_codebooks: null %s", !b ? "pq rows" : "out"); return LEANN_ERR_INVALID; }
    memcpy(out, b->cb_host.data(), b->cb_host.size() * 4);
    return LEANN_OK;
}
extern "C" int leann_pq_rows_export(const leann_pq_rows *b, uint8_t *out) {
    if (!b || (!out && b->n)) { leann_set_error("leann_pq_rows_export: null %s", !b ? "pq rows" : "out"); return LEANN_ERR_INVALID; }
    if (b->n == 0) return LEANN_OK;
    HIP_CHECK_RET(hipSetDevice(b->device));
    const size_t MP = b->sh.MP, NS = b->sh.NS, slab = (size_t)1 << 20; // rows copied out at a time, whole blocks
    std::vector<uint8_t> tmp(std::min(slab, pq_rows64(b->n)) * MP);
    for (size_t r0 = 0; r0 < b->n; r0 += slab) {
        const size_t rows = std::min(slab, b->n - r0);
        HIP_CHECK_RET(hipMemcpy(tmp.data(), b->codes.p + r0 * MP, pq_rows64(rows) * MP, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < rows; i++)
            for (size_t m = 0; m < MP; m++) out[(r0 + i) * MP + m] = tmp[pq_code_at(i, m, NS)];
    }
    return LEANN_OK;
}
extern "C" void leann_pq_rows_close(leann_pq_rows *b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    (void)hipDeviceSynchronize(); // no kernel still reads the codes
    delete b;
}

// ---- the query tables -----------------------------------------------------------------------------------------------------------------
// grid = nq rounded up to PQ_BQ; W [groups][MP][256][PQ_BQ] int16: the entry of (m, c) for the 8 queries of a group is 16 contiguous
// bytes.  Tables of padding sub-spaces, of padding queries and of a query without tables are zero; bad [nq]: 1 for the latter.
template <int DSUB>
__global__ void __launch_bounds__(256) pq_lut_kernel(const float *__restrict__ Q, uint32_t nq, uint32_t d, const float *__restrict__ C,
                                                     uint32_t M, uint32_t MP, int16_t *__restrict__ W, uint32_t *__restrict__ bad) {
    __shared__ float sq[PQ_MAX_DIMS + 8];
    __shared__ uint32_t s_max, s_qbad;
    const uint32_t q = blockIdx.x, c = threadIdx.x;
    int16_t *out = W + ((size_t)(q / PQ_BQ) * MP * 256) * PQ_BQ + q % PQ_BQ; // entry (m, c) at out[(m 256 + c) PQ_BQ]
    if (q >= nq) {
        for (uint32_t m = 0; m < MP; m++) out[((size_t)m * 256 + c) * PQ_BQ] = 0;
        return;
    }
    if (c == 0) s_max = 0u, s_qbad = 0u;
    __syncthreads();
    for (uint32_t j = c; j < M * DSUB; j += 256) {
        const float v = j < d ? Q[(size_t)q * d + j] : 0.f;
        if (!pq_finite(v)) atomicOr(&s_qbad, 1u);
        sq[j] = v;
    }
    __syncthreads();
    uint32_t mb = 0; // bits of max |L| over this thread's entries: a NaN or an infinity is >= 0x7F800000
    for (uint32_t m = 0; m < M; m++)
        mb = max(mb, __float_as_uint((float)pq_dot<DSUB>(sq + m * DSUB, C + ((size_t)m * 256 + c) * DSUB)) & 0x7FFFFFFFu);
    atomicMax(&s_max, mb);
    __syncthreads();
    const bool ok = !s_qbad && s_max < 0x7F800000u;
    if (c == 0) bad[q] = ok ? 0u : 1u;
    const uint32_t E = max(s_max >> 23, 1u);
    for (uint32_t m = 0; m < MP; m++) {
        int w = 0;
        if (ok && m < M) w = pq_entry((float)pq_dot<DSUB>(sq + m * DSUB, C + ((size_t)m * 256 + c) * DSUB), E);
        out[((size_t)m * 256 + c) * PQ_BQ] = (int16_t)w;
    }
}

// ---- the score --------------------------------------------------------------------------------------------------------------------------
// Two 16-bit entries of a table dword into their two 32-bit accumulators.  Of the three forms the issue names, the ISA of this file
// decides: 0 = sign-extending extracts and adds as the compiler selects them, 1 = v_dot2_i32_i16 with the selectors
// (1, 0) and (0, 1), one instruction per entry.
#ifndef PQ_ACC
#define PQ_ACC 1
#endif
__device__ __forceinline__ void pq_acc2(int &a0, int &a1, int e) {
#if PQ_ACC == 1
    const i16x2 v = __builtin_bit_cast(i16x2, e), lo = {1, 0}, hi = {0, 1};
    a0 = __builtin_amdgcn_sdot2(v, lo, a0, false);
    a1 = __builtin_amdgcn_sdot2(v, hi, a1, false);
#else
    a0 += (int)(short)(e & 0xFFFF);
    a1 += e >> 16;
#endif
}

// LIST: row i of the launch is store row idx[row0 + i] (the allowed positions, compacted ascending); scores, slab columns and emitted
// keys are then indexed by i, and finalize_scan_kernel (scan.hip) maps i -> idx[i].  Output: score_mx4_mfma_kernel's contract, an f32
// slab S[q n_rows + row] or CandEmit emission.  grid.x = row tiles x query groups, the group running fastest: the workgroups that
// stream one row tile's codes are neighbours in time.
template <bool LIST>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) score_pq_kernel(const uint8_t *__restrict__ codes, uint32_t NS, uint64_t n_store,
                                                       const int16_t *__restrict__ W, uint32_t nq, uint32_t groups, uint64_t row0,
                                                       uint32_t n_rows, float *__restrict__ S /* [nq x n_rows] */, CandEmit em,
                                                       const uint32_t *__restrict__ idx) {
    constexpr int SL = PQ_MS * 256, TP = SL / 256; // 16-B slots of a slice; staging passes of a thread
    __shared__ i32x4 sT[2 * SL];
    const uint32_t tid = threadIdx.x, g = blockIdx.x % groups, rbase = (blockIdx.x / groups) * PQ_BR;
    int acc[PQ_RPT][PQ_BQ];
#pragma unroll
    for (int r = 0; r < (int)PQ_RPT; r++)
#pragma unroll
        for (int q = 0; q < (int)PQ_BQ; q++) acc[r][q] = 0;
    const uint8_t *cp[PQ_RPT];
#pragma unroll
    for (int r = 0; r < (int)PQ_RPT; r++) { // checked before it becomes an address; rows past the launch are clamped to its last row
        const uint32_t row = min(rbase + 256 * r + tid, n_rows - 1);
        const uint64_t sr = min(LIST ? (uint64_t)idx[row0 + row] : row0 + row, n_store - 1);
        cp[r] = codes + ((sr >> 6) * NS * 64 + (sr & 63)) * 8;
    }
    const i32x4 *tp = reinterpret_cast<const i32x4 *>(W) + (size_t)g * NS * SL + tid;
    uint2 cv[PQ_RPT];
    i32x4 tv[TP];
    auto gload = [&](uint32_t s) {
#pragma unroll
        for (int r = 0; r < (int)PQ_RPT; r++) cv[r] = *reinterpret_cast<const uint2 *>(cp[r] + (size_t)s * 512);
#pragma unroll
        for (int p = 0; p < TP; p++) tv[p] = tp[(size_t)s * SL + 256 * p];
    };
    gload(0);
#pragma unroll
    for (int p = 0; p < TP; p++) sT[256 * p + tid] = tv[p];
    __syncthreads();
    for (uint32_t s = 0; s < NS; s++) {
        uint2 cc[PQ_RPT];
#pragma unroll
        for (int r = 0; r < (int)PQ_RPT; r++) cc[r] = cv[r];
        gload(min(s + 1, NS - 1)); // no branch in the loop body (the last pass loads its own slice again and nobody reads it): one
                                   // basic block, so the barriers below bound what the scheduler keeps in flight
        const i32x4 *T = sT + (s & 1u) * SL;
#pragma unroll
        for (int r = 0; r < (int)PQ_RPT; r++) {
#pragma unroll
            for (int mm = 0; mm < (int)PQ_MS; mm++) {
                const uint32_t code = ((mm < 4 ? cc[r].x : cc[r].y) >> (8 * (mm & 3))) & 255u;
                const i32x4 e = T[256 * mm + code];
                pq_acc2(acc[r][0], acc[r][1], e[0]);
                pq_acc2(acc[r][2], acc[r][3], e[1]);
                pq_acc2(acc[r][4], acc[r][5], e[2]);
                pq_acc2(acc[r][6], acc[r][7], e[3]);
            }
            __builtin_amdgcn_sched_barrier(0); // one row's 8 reads in flight at a time: hoisting all 64 spilled 200 VGPRs
        }
        i32x4 *Tn = sT + ((s + 1) & 1u) * SL; // the other buffer: its readers passed the barrier of slice s - 1
#pragma unroll
        for (int p = 0; p < TP; p++) Tn[256 * p + tid] = tv[p];
        __syncthreads();
    }
    const uint32_t qbase = g * PQ_BQ;
    if (em.thr) { // candidate emission (CandEmit, internal.h); a padding query of the last group (q >= nq) never emits
        float thr[PQ_BQ];
#pragma unroll
        for (int q = 0; q < (int)PQ_BQ; q++) thr[q] = qbase + q < nq ? em.thr[qbase + q] : __uint_as_float(0x7F800000u);
#pragma unroll
        for (int r = 0; r < (int)PQ_RPT; r++) {
            const uint32_t row = rbase + 256 * r + tid;
            bool any = false;
#pragma unroll
            for (int q = 0; q < (int)PQ_BQ; q++) any |= qbase + q < nq && (float)acc[r][q] >= thr[q];
            if (!any || row >= n_rows) continue;
            const uint64_t pos = em.pos0 + row;
            if (em.allow && !((em.allow[pos >> 3] >> (pos & 7)) & 1)) continue;
#pragma unroll
            for (int q = 0; q < (int)PQ_BQ; q++) {
                const float sv = (float)acc[r][q];
                if (qbase + q < nq && sv >= thr[q]) {
                    const uint32_t slot = atomicAdd(&em.cnt[qbase + q], 1u);
                    if (slot < em.cap) em.list[(size_t)(qbase + q) * em.cap + slot] = ((uint64_t)(~f32_orderable(sv)) << 32) | (uint32_t)pos;
                }
            }
        }
        return;
    }
#pragma unroll
    for (int r = 0; r < (int)PQ_RPT; r++) {
        const uint32_t row = rbase + 256 * r + tid;
        if (row < n_rows)
#pragma unroll
            for (int q = 0; q < (int)PQ_BQ; q++)
                if (qbase + q < nq) S[(size_t)(qbase + q) * n_rows + row] = (float)acc[r][q];
    }
}

static void launch_score_pq(hipStream_t st, const leann_pq_rows *b, const int16_t *W, size_t nq, size_t row0, size_t rows, float *S,
                            const CandEmit &em, const uint32_t *idx) {
    const uint32_t groups = (uint32_t)(pq_query_rows(nq) / PQ_BQ);
    const dim3 grid((unsigned)((rows + PQ_BR - 1) / PQ_BR * groups));
    if (idx)
        hipLaunchKernelGGL(score_pq_kernel<true>, grid, dim3(256), 0, st, b->codes.p, (uint32_t)b->sh.NS, (uint64_t)b->n, W, (uint32_t)nq, groups,
                           (uint64_t)row0, (uint32_t)rows, S, em, idx);
    else
        hipLaunchKernelGGL(score_pq_kernel<false>, grid, dim3(256), 0, st, b->codes.p, (uint32_t)b->sh.NS, (uint64_t)b->n, W, (uint32_t)nq, groups,
                           (uint64_t)row0, (uint32_t)rows, S, em, idx);
}

// grid = nq; a query without tables (bad[q], or every query when bad == null: no row is allowed) has count 0 and nothing but tail
__global__ void __launch_bounds__(64) pq_no_answer_kernel(const uint32_t *__restrict__ bad, uint32_t k, uint64_t *__restrict__ keys,
                                                          float *__restrict__ scores, uint32_t *__restrict__ counts) {
    const uint32_t q = blockIdx.x;
    if (bad && !bad[q]) return;
    for (uint32_t i = threadIdx.x; i < k; i += 64) {
        keys[(size_t)q * k + i] = ~0ull;
        scores[(size_t)q * k + i] = __uint_as_float(0xFF800000u); // -inf: the tail value of topk_finish's scores
    }
    if (threadIdx.x == 0) counts[q] = 0;
}

// ---- host side --------------------------------------------------------------------------------------------------------------------------
// Follows mx4_run (scan_mx4.hip): plan, leases, begin, per chunk { score, select }, finish — which writes keys and scores straight
// into the caller's arrays —, once more on the slab schedule if a candidate list overflowed.  Returns with `st` synchronised.
static int pq_run(const leann_pq_rows *b, const float *d_queries, size_t nq, size_t fetch_k, const uint8_t *d_allow, uint64_t *d_keys,
                  float *d_scores, uint32_t *d_counts, hipStream_t st) {
    const uint32_t k = (uint32_t)fetch_k;
    const size_t nq_pad = pq_query_rows(nq);
    const PqShape &sh = b->sh;
    // every return, early ones included, gives the scratch back — after the stream is idle (SyncFirst is declared last, so it runs first)
    ScratchLease<int16_t> W;
    ScratchLease<uint32_t> bad, list;
    struct SyncFirst {
        hipStream_t st;
        ~SyncFirst() { (void)hipStreamSynchronize(st); }
    } sync_first{st};
    if (int e = W.acquire(nq_pad * sh.MP * 256)) return e;
    if (int e = bad.acquire(nq)) return e;
    if (sh.dsub == 4)
        hipLaunchKernelGGL(pq_lut_kernel<4>, dim3((unsigned)nq_pad), dim3(256), 0, st, d_queries, (uint32_t)nq, (uint32_t)sh.dims, b->cb.p,
                           (uint32_t)sh.M, (uint32_t)sh.MP, W.p, bad.p);
    else
        hipLaunchKernelGGL(pq_lut_kernel<8>, dim3((unsigned)nq_pad), dim3(256), 0, st, d_queries, (uint32_t)nq, (uint32_t)sh.dims, b->cb.p,
                           (uint32_t)sh.M, (uint32_t)sh.MP, W.p, bad.p);
    HIP_CHECK_RET(hipGetLastError());
    // the rows of the search: all of them, or the allowed ones as an ascending list
    size_t m = b->n;
    if (d_allow)
        if (int rc = leann_internal_compact_allow(d_allow, b->n, &list, &m, st)) return rc;
    const uint32_t *idx = d_allow ? list.p : nullptr;
    const TopkShape shape = topk_shape_scan(m, nq, k);
    for (bool emit = m > shape.emit_first && !leann_knobs().no_emit; m != 0; emit = false) {
        TopkRun run{topk_plan(shape, emit)};
        const TopkPlan &p = run.plan;
        ScratchLease<float> S;
        ScratchLease<uint64_t> candA, candB, best;
        ScratchLease<unsigned char> emb;
        SyncFirst sync_pass{st};
        if (int e = S.acquire(shape.q_tile * p.slab_rows)) return e;
        if (int e = candA.acquire(nq * p.cand_len)) return e;
        if (int e = candB.acquire(nq * p.cand_len)) return e;
        if (int e = best.acquire(nq * k)) return e;
        if (p.emit)
            if (int e = emb.acquire(p.emit_bytes)) return e;
        run.S = S, run.candA = candA, run.candB = candB, run.best = best, run.emit_block = emb;
        run.nq = nq, run.k = k, run.allow = nullptr, run.st = st;
        int rc = leann_internal_topk_begin(run);
        for (size_t c = 0; c < p.chunks.size() && rc == LEANN_OK; c++) {
            launch_score_pq(st, b, W, nq, p.chunks[c].first, p.chunks[c].second, S, run.chunk_emit(c), idx);
            rc = leann_internal_topk_select_chunk(run, c, 0, (uint32_t)nq);
        }
        bool overflowed = false;
        if (rc == LEANN_OK) rc = leann_internal_topk_finish(run, b->key_offset, idx, 0, d_keys, d_scores, d_counts, &overflowed);
        if (rc != LEANN_OK) return rc;
        if (!overflowed) break;
    }
    hipLaunchKernelGGL(pq_no_answer_kernel, dim3((unsigned)nq), dim3(64), 0, st, m ? bad.p : nullptr, k, d_keys, d_scores, d_counts);
    HIP_CHECK_RET(hipGetLastError());
    HIP_CHECK_RET(hipStreamSynchronize(st));
    return LEANN_OK;
}

// what the entry points refuse, on the host, before any device work
static int pq_check(const char *who, const leann_pq_rows *b, const void *queries, size_t nq, size_t fetch_k, const void *keys,
                    const void *out2, const char *out2_name, const void *counts) {
    if (!b || (nq && (!queries || !keys || !out2 || !counts))) {
        leann_set_error("%s: null %s", who, !b ? "pq rows" : !queries ? "queries" : !keys ? "keys" : !out2 ? out2_name : "counts");
        return LEANN_ERR_INVALID;
    }
    if (fetch_k < 1 || fetch_k > PQ_MAX_K) { leann_set_error("%s: fetch_k = %zu is outside [1, %zu]", who, fetch_k, PQ_MAX_K); return LEANN_ERR_INVALID; }
    if (nq >= (1ull << 31)) { leann_set_error("%s: nq = %zu is 2^31 or more", who, nq); return LEANN_ERR_INVALID; }
    return LEANN_OK;
}
static int pq_refined_check(const char *who, const leann_pq_rows *b, const leann_exact_rows *r, const void *queries, size_t nq, size_t top_k,
                            size_t fetch_k, const void *keys, const void *dists, const void *counts) {
    if (!r) { leann_set_error("%s: null exact rows", who); return LEANN_ERR_INVALID; }
    if (int rc = pq_check(who, b, queries, nq, fetch_k, keys, dists, "dists", counts)) return rc;
    if (top_k < 1) { leann_set_error("%s: top_k = 0", who); return LEANN_ERR_INVALID; }
    if (top_k > fetch_k) { leann_set_error("%s: top_k = %zu is above fetch_k = %zu", who, top_k, fetch_k); return LEANN_ERR_INVALID; }
    if (r->dims != b->sh.dims) { leann_set_error("%s: the exact rows have dims = %zu, the pq rows %zu", who, r->dims, b->sh.dims); return LEANN_ERR_INVALID; }
    if (r->device != b->device) {
        leann_set_error("%s: the exact rows are on device %d, the pq rows on device %d", who, r->device, b->device);
        return LEANN_ERR_INVALID;
    }
    if (r->key_offset > b->key_offset || b->key_offset + b->n > r->key_offset + r->n) {
        leann_set_error("%s: the exact rows cover positions [%llu, %llu), the pq rows need key_offset .. key_offset + len = [%llu, %llu)", who,
                        (unsigned long long)r->key_offset, (unsigned long long)(r->key_offset + r->n), (unsigned long long)b->key_offset,
                        (unsigned long long)(b->key_offset + b->n));
        return LEANN_ERR_INVALID;
    }
    return LEANN_OK;
}
// an empty object: every answer is empty
static int pq_run_or_empty(const leann_pq_rows *b, const float *d_queries, size_t nq, size_t fetch_k, const uint8_t *d_allow, uint64_t *d_keys,
                           float *d_scores, uint32_t *d_counts, hipStream_t st) {
    if (b->n) return pq_run(b, d_queries, nq, fetch_k, d_allow, d_keys, d_scores, d_counts, st);
    hipLaunchKernelGGL(pq_no_answer_kernel, dim3((unsigned)nq), dim3(64), 0, st, (const uint32_t *)nullptr, (uint32_t)fetch_k, d_keys, d_scores,
                       d_counts);
    HIP_CHECK_RET(hipGetLastError());
    HIP_CHECK_RET(hipStreamSynchronize(st));
    return LEANN_OK;
}

extern "C" int leann_pq_rows_search_batch_device(const leann_pq_rows *b, const float *d_queries, size_t nq, size_t fetch_k,
                                                 const uint8_t *d_allow, uint64_t *d_keys, float *d_scores, uint32_t *d_counts, void *stream) {
    if (int rc = pq_check("leann_pq_rows_search_batch_device", b, d_queries, nq, fetch_k, d_keys, d_scores, "scores", d_counts)) return rc;
    if (nq == 0) return LEANN_OK;
    HIP_CHECK_RET(hipSetDevice(b->device));
    return pq_run_or_empty(b, d_queries, nq, fetch_k, d_allow, d_keys, d_scores, d_counts, (hipStream_t)stream);
}

// The candidates into library scratch, then the rerank on the same stream.
static int pq_refined_run(const char *who, const leann_pq_rows *b, const leann_exact_rows *r, const float *d_queries, size_t nq, size_t top_k,
                          size_t fetch_k, const uint8_t *d_allow, uint64_t *d_keys, float *d_dists, uint32_t *d_counts, hipStream_t st) {
    ScratchLease<uint64_t> w_keys;
    ScratchLease<float> w_scores;
    ScratchLease<uint32_t> w_counts;
    if (int e = w_keys.acquire(nq * fetch_k)) return e;
    if (int e = w_scores.acquire(nq * fetch_k)) return e;
    if (int e = w_counts.acquire(nq)) return e;
    int rc = pq_run_or_empty(b, d_queries, nq, fetch_k, d_allow, w_keys, w_scores, w_counts, st);
    if (rc == LEANN_OK) rc = leann_rerank_batch_device(r, d_queries, nq, w_keys, w_counts, fetch_k, top_k, d_keys, d_dists, d_counts, nullptr, st);
    // the leases end with the call: nothing may still be reading the lists
    if (hipStreamSynchronize(st) != hipSuccess && rc == LEANN_OK) {
        leann_set_error("%s: the search or the rerank failed on the device", who);
        rc = LEANN_ERR_DEVICE;
    }
    return rc;
}

extern "C" int leann_pq_rows_search_refined_batch_device(const leann_pq_rows *b, const leann_exact_rows *r, const float *d_queries, size_t nq,
                                                         size_t top_k, size_t fetch_k, const uint8_t *d_allow, uint64_t *d_keys,
                                                         float *d_dists, uint32_t *d_counts, void *stream) {
    const char *who = "leann_pq_rows_search_refined_batch_device";
    if (int rc = pq_refined_check(who, b, r, d_queries, nq, top_k, fetch_k, d_keys, d_dists, d_counts)) return rc;
    if (nq == 0) return LEANN_OK;
    HIP_CHECK_RET(hipSetDevice(b->device));
    return pq_refined_run(who, b, r, d_queries, nq, top_k, fetch_k, d_allow, d_keys, d_dists, d_counts, (hipStream_t)stream);
}

// the host-pointer twins: r == null is the plain search (k_out = fetch_k scores), else the refined one (k_out = top_k distances)
static int pq_host_call(const char *who, const leann_pq_rows *b, const leann_exact_rows *r, const float *queries, size_t nq, size_t top_k,
                        size_t fetch_k, const uint8_t *allow, uint64_t *keys, float *out2, uint32_t *counts) {
    if (nq == 0) return LEANN_OK;
    HIP_CHECK_RET(hipSetDevice(b->device));
    const size_t k_out = r ? top_k : fetch_k;
    DeviceBuf<float> d_q, d_out2;
    DeviceBuf<uint64_t> d_keys;
    DeviceBuf<uint32_t> d_counts;
    DeviceBuf<uint8_t> d_allow;
    if (int rc = d_q.alloc(nq * b->sh.dims)) return rc;
    if (int rc = d_keys.alloc(nq * k_out)) return rc;
    if (int rc = d_out2.alloc(nq * k_out)) return rc;
    if (int rc = d_counts.alloc(nq)) return rc;
    HIP_CHECK_RET(hipMemcpy(d_q, queries, nq * b->sh.dims * 4, hipMemcpyHostToDevice));
    if (allow && b->n) {
        if (int rc = d_allow.alloc((b->n + 7) / 8)) return rc;
        HIP_CHECK_RET(hipMemcpy(d_allow, allow, (b->n + 7) / 8, hipMemcpyHostToDevice));
    }
    const uint8_t *da = allow && b->n ? d_allow.p : nullptr;
    if (int rc = r ? pq_refined_run(who, b, r, d_q, nq, top_k, fetch_k, da, d_keys, d_out2, d_counts, nullptr)
                   : pq_run_or_empty(b, d_q, nq, fetch_k, da, d_keys, d_out2, d_counts, nullptr))
        return rc;
    HIP_CHECK_RET(hipMemcpy(keys, d_keys, nq * k_out * 8, hipMemcpyDeviceToHost));
    HIP_CHECK_RET(hipMemcpy(out2, d_out2, nq * k_out * 4, hipMemcpyDeviceToHost));
    HIP_CHECK_RET(hipMemcpy(counts, d_counts, nq * 4, hipMemcpyDeviceToHost));
    return LEANN_OK;
}

extern "C" int leann_pq_rows_search_batch(const leann_pq_rows *b, const float *queries, size_t nq, size_t fetch_k, const uint8_t *allow,
                                          uint64_t *keys, float *scores, uint32_t *counts) {
    const char *who = "leann_pq_rows_search_batch";
    if (int rc = pq_check(who, b, queries, nq, fetch_k, keys, scores, "scores", counts)) return rc;
    return pq_host_call(who, b, nullptr, queries, nq, 0, fetch_k, allow, keys, scores, counts);
}

extern "C" int leann_pq_rows_search_refined_batch(const leann_pq_rows *b, const leann_exact_rows *r, const float *queries, size_t nq,
                                                  size_t top_k, size_t fetch_k, const uint8_t *allow, uint64_t *keys, float *dists,
                                                  uint32_t *counts) {
    const char *who = "leann_pq_rows_search_refined_batch";
    if (int rc = pq_refined_check(who, b, r, queries, nq, top_k, fetch_k, keys, dists, counts)) return rc;
    return pq_host_call(who, b, r, queries, nq, top_k, fetch_k, allow, keys, dists, counts);
}

// ---- the trainer ------------------------------------------------------------------------------------------------------------------------
// grid = M; centroid c of sub-space m = sub-vector m of row floor(c n / 256), what is not finite and padding columns as 0
__global__ void __launch_bounds__(256) pq_init_centroids_kernel(const float *__restrict__ X, uint64_t n, uint32_t d, uint64_t ld, uint32_t dsub,
                                                                float *__restrict__ C) {
    const uint32_t m = blockIdx.x, c = threadIdx.x;
    const float *x = X + ((uint64_t)c * n / 256) * ld;
    for (uint32_t j = 0; j < dsub; j++) {
        const uint32_t col = m * dsub + j;
        C[((size_t)m * 256 + c) * dsub + j] = col < d ? pq_clean(x[col]) : 0.f;
    }
}
// grid = (M, DSUB); thread c of block (m, j) owns column j of centroid c: it walks the samples in order, 256 at a time through LDS
// (each thread stages one code byte and one element), and sums its members in float64 — the same order, hence the same bytes, on
// every run.  A centroid without members keeps its value.
template <int DSUB>
__global__ void __launch_bounds__(256) pq_update_kernel(const float *__restrict__ X, uint64_t n, uint32_t d, uint64_t ld,
                                                        const uint8_t *__restrict__ codes, uint32_t NS, float *__restrict__ C) {
    __shared__ uint32_t sc[256];
    __shared__ float sx[256];
    const uint32_t m = blockIdx.x, j = blockIdx.y, c = threadIdx.x, col = m * DSUB + j;
    double sum = 0.0;
    uint32_t count = 0;
    for (uint64_t i0 = 0; i0 < n; i0 += 256) {
        const uint64_t i = i0 + c;
        __syncthreads();
        sc[c] = i < n ? codes[(((i >> 6) * NS + (m >> 3)) * 64 + (i & 63)) * 8 + (m & 7)] : 0u;
        sx[c] = i < n && col < d ? pq_clean(X[i * ld + col]) : 0.f;
        __syncthreads();
        const uint32_t lim = (uint32_t)min((uint64_t)256, n - i0);
        for (uint32_t t = 0; t < lim; t++)
            if (sc[t] == c) {
                sum = sum + (double)sx[t];
                count++;
            }
    }
    if (count) C[((size_t)m * 256 + c) * DSUB + j] = (float)(sum / (double)count);
}

static int pq_train_check(const char *who, const void *rows, const char *rows_name, size_t n, size_t dims, size_t dsub, int device, const void *out) {
    if (!rows || !out) { leann_set_error("%s: null %s", who, !rows ? rows_name : "codebooks_out"); return LEANN_ERR_INVALID; }
    if (int rc = pq_check_shape(who, dims, dsub)) return rc;
    if (n < 256 || n >= 0xFFFFFFFFull) { leann_set_error("%s: n = %zu is outside [256, 2^32 - 1)", who, n); return LEANN_ERR_INVALID; }
    if (device < 0) { leann_set_error("%s: device = %d", who, device); return LEANN_ERR_INVALID; }
    return LEANN_OK;
}
static int pq_train_run(const float *d_rows, size_t n, const PqShape &sh, size_t ld, size_t iters, float *codebooks_out) {
    DeviceBuf<float> cb;
    DeviceBuf<uint8_t> codes;
    if (int rc = cb.alloc(sh.M * 256 * sh.dsub)) return rc;
    if (iters)
        if (int rc = codes.alloc(pq_rows64(n) * sh.MP)) return rc;
    hipLaunchKernelGGL(pq_init_centroids_kernel, dim3((unsigned)sh.M), dim3(256), 0, nullptr, d_rows, (uint64_t)n, (uint32_t)sh.dims, (uint64_t)ld,
                       (uint32_t)sh.dsub, cb.p);
    HIP_CHECK_RET(hipGetLastError());
    for (size_t it = 0; it < iters; it++) {
        pq_launch_encode(d_rows, n, sh, ld, cb, codes);
        HIP_CHECK_RET(hipGetLastError());
        const dim3 grid((unsigned)sh.M, (unsigned)sh.dsub);
        if (sh.dsub == 4)
            hipLaunchKernelGGL(pq_update_kernel<4>, grid, dim3(256), 0, nullptr, d_rows, (uint64_t)n, (uint32_t)sh.dims, (uint64_t)ld, codes.p,
                               (uint32_t)sh.NS, cb.p);
        else
            hipLaunchKernelGGL(pq_update_kernel<8>, grid, dim3(256), 0, nullptr, d_rows, (uint64_t)n, (uint32_t)sh.dims, (uint64_t)ld, codes.p,
                               (uint32_t)sh.NS, cb.p);
        HIP_CHECK_RET(hipGetLastError());
    }
    HIP_CHECK_RET(hipMemcpy(codebooks_out, cb, sh.M * 256 * sh.dsub * 4, hipMemcpyDeviceToHost)); // waits for the kernels
    return LEANN_OK;
}

extern "C" int leann_pq_train_device(const float *d_rows, size_t n, size_t dims, size_t ld, size_t dsub, size_t iters, int device,
                                     float *codebooks_out) {
    const char *who = "leann_pq_train_device";
    if (int rc = pq_train_check(who, d_rows, "d_rows", n, dims, dsub, device, codebooks_out)) return rc;
    if (ld < dims) { leann_set_error("%s: ld = %zu is below dims = %zu", who, ld, dims); return LEANN_ERR_INVALID; }
    if (int rc = leann_internal_check_device(device)) return rc;
    HIP_CHECK_RET(hipSetDevice(device));
    return pq_train_run(d_rows, n, pq_shape(dims, dsub), ld, iters, codebooks_out);
}

extern "C" int leann_pq_train(const float *rows, size_t n, size_t dims, size_t dsub, size_t iters, int device, float *codebooks_out) {
    const char *who = "leann_pq_train";
    if (int rc = pq_train_check(who, rows, "rows", n, dims, dsub, device, codebooks_out)) return rc;
    if (int rc = leann_internal_check_device(device)) return rc;
    HIP_CHECK_RET(hipSetDevice(device));
    DeviceBuf<float> d_rows; // the caller subsamples: the sample is expected to fit
    if (int rc = d_rows.alloc(n * dims)) return rc;
    HIP_CHECK_RET(hipMemcpy(d_rows, rows, n * dims * 4, hipMemcpyHostToDevice));
    return pq_train_run(d_rows, n, pq_shape(dims, dsub), dims, iters, codebooks_out);
}
