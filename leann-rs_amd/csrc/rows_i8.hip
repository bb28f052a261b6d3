// rows_i8.hip — graph indexes whose rows are int8 codes with one power-of-two scale per column (LEANN_ROWS_I8,
// include/leann_backend.h; DESIGN.md "int8 rows").
//
// Definition (i8_rows.h): amax_j = max_i |x_ij|, e_j the largest integer in [-32, 32] with amax_j 2^e_j <= 127 (0 for a zero column),
// c_ij = clamp(rne(x_ij 2^e_j), -127, 127), Xq_ij = (float)c_ij 2^-e_j.  An int8 index over rows X is the f32 index over Xq with the
// same graph, bit for bit.  The search kernels are search_i8.hip's; this file holds the row store — the column reduction and the
// quantising kernel on the device, the way in from host rows, device rows and index files, the way out — and the row-type entry
// points' int8 branches (rows_bf16.hip owns the entry points themselves).
//
// Device layout: [n x ldb] bytes, ldb = dims rounded up to 128, zero padded — a row is whole, aligned 128-B lines (768-d: 6) — with
// the elements in i8_row_pos order (i8_rows.h).  g.X names the store, g.row_bytes = ldb; g.ld keeps the f32 meaning (dims rounded up to
// 4) and selects the kernel; g.norms names the column scales 2^-e_j, f32 [g.ld], padding 1.0.  The exponents stay on the host
// (leann_backend::i8_exps).  Files and exports are in plain element order.
#include "common.cuh"
#include "internal.h"
#include "i8_rows.h"

#include <algorithm>
#include <new>
#include <vector>

// Column reduction.  amax_bits[j] = max over the rows of the bits of |x_ij| (non-negative floats order as their bits do; a NaN or an
// infinity is >= 0x7F800000 and larger than every finite value); first_bad = the smallest row-major index row * d + j of a
// non-finite element (row0 = the index of X's first row in the whole matrix).  Work item (blockIdx.x * 256 + threadIdx.x) owns
// the four columns 4 c .. 4 c + 3 over the rows blockIdx.y, + gridDim.y, ..: a wave reads 1 KiB of one row per instruction.
__global__ void __launch_bounds__(256) i8_column_amax_kernel(const float *__restrict__ X, uint64_t n, uint32_t d, uint32_t ld, uint64_t row0,
                                                             uint32_t *__restrict__ amax_bits /* [ld] */, unsigned long long *first_bad) {
    const uint32_t j = (blockIdx.x * 256u + threadIdx.x) << 2;
    if (j >= ld) return; // ld is a multiple of 4
    uint32_t m[4] = {0u, 0u, 0u, 0u};
    unsigned long long bad = ~0ull;
    for (uint64_t row = blockIdx.y; row < n; row += gridDim.y) {
        const float4 v = *reinterpret_cast<const float4 *>(X + row * ld + j);
        const uint32_t b[4] = {__float_as_uint(v.x) & 0x7FFFFFFFu, __float_as_uint(v.y) & 0x7FFFFFFFu, __float_as_uint(v.z) & 0x7FFFFFFFu,
                               __float_as_uint(v.w) & 0x7FFFFFFFu};
#pragma unroll
        for (int e = 0; e < 4; e++) {
            if (j + e >= d) continue; // padding: whatever X holds there is not data
            m[e] = max(m[e], b[e]);
            if (b[e] >= 0x7F800000u) bad = min(bad, (unsigned long long)(row0 + row) * d + j + e);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; e++)
        if (m[e]) atomicMax(amax_bits + j + e, m[e]);
    if (bad != ~0ull) atomicMin(first_bad, bad);
}

// one work item = four elements 4 i .. 4 i + 3 of a store row (contiguous in X and — i8_row_pos keeps groups of four together — in the
// store).  scale_up = 2^e_j, scale_down = 2^-e_j, both [ld].  out: the store (may be null); deq: Xq written back over X (may be null:
// leann_backend_build_device_rows builds on the dequantised rows).
__global__ void __launch_bounds__(256) quantize_rows_i8_kernel(const float *X, uint64_t n, uint32_t d, uint32_t ld, uint32_t ldb,
                                                               const float *__restrict__ scale_up, const float *__restrict__ scale_down,
                                                               int8_t *__restrict__ out, float *deq /* may be X itself */) {
    const uint32_t per_row = ldb >> 2;
    const uint64_t items = n * per_row;
    for (uint64_t it = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t row = it / per_row;
        const uint32_t j = (uint32_t)(it - row * per_row) << 2;
        int8_t c[4] = {0, 0, 0, 0};
        if (j < ld) { // ld is a multiple of 4: the group is inside the row or padding
            const float4 v = *reinterpret_cast<const float4 *>(X + row * ld + j);
            const float4 up = *reinterpret_cast<const float4 *>(scale_up + j);
            c[0] = j + 0 < d ? i8_code(v.x, up.x) : (int8_t)0; // (elements past dims are padding: zero in the store whatever X holds)
            c[1] = j + 1 < d ? i8_code(v.y, up.y) : (int8_t)0;
            c[2] = j + 2 < d ? i8_code(v.z, up.z) : (int8_t)0;
            c[3] = j + 3 < d ? i8_code(v.w, up.w) : (int8_t)0;
            if (deq) {
                const float4 dn = *reinterpret_cast<const float4 *>(scale_down + j);
                *reinterpret_cast<float4 *>(deq + row * ld + j) =
                    make_float4((float)c[0] * dn.x, (float)c[1] * dn.y, (float)c[2] * dn.z, (float)c[3] * dn.w);
            }
        }
        if (out)
            *reinterpret_cast<uint32_t *>(out + (size_t)row * ldb + i8_row_pos(j, ldb)) =
                (uint32_t)(uint8_t)c[0] | ((uint32_t)(uint8_t)c[1] << 8) | ((uint32_t)(uint8_t)c[2] << 16) | ((uint32_t)(uint8_t)c[3] << 24);
    }
}

// ---- the column pass: amax and the first non-finite element of device rows, accumulated over slabs ------------------------------------
struct ColumnPass {
    DeviceBuf<uint32_t> amax;            // [ld] bits
    DeviceBuf<unsigned long long> bad;   // [1]
    uint32_t d = 0, ld = 0;
    int begin(uint32_t d_, uint32_t ld_) {
        d = d_; ld = ld_;
        if (amax.alloc(ld) || bad.alloc(1)) return LEANN_ERR_DEVICE;
        HIP_CHECK_RET(hipMemset(amax, 0, (size_t)ld * 4));
        HIP_CHECK_RET(hipMemset(bad, 0xFF, 8));
        return LEANN_OK;
    }
    int add(const float *d_rows, size_t n, size_t row0) const {
        if (n == 0) return LEANN_OK;
        const unsigned gx = (ld / 4 + 255) / 256, gy = (unsigned)std::min<size_t>(n, 2048);
        hipLaunchKernelGGL(i8_column_amax_kernel, dim3(gx, gy), dim3(256), 0, nullptr, d_rows, (uint64_t)n, d, ld, (uint64_t)row0, amax.p, bad.p);
        HIP_CHECK_RET(hipGetLastError());
        return LEANN_OK;
    }
    // exps [d]; LEANN_ERR_INVALID naming the first non-finite element
    int finish(const char *who, std::vector<int8_t> *exps) const {
        std::vector<uint32_t> bits(ld);
        unsigned long long first = 0;
        HIP_CHECK_RET(hipDeviceSynchronize()); // null-stream work
        HIP_CHECK_RET(hipMemcpy(bits.data(), amax, (size_t)ld * 4, hipMemcpyDeviceToHost));
        HIP_CHECK_RET(hipMemcpy(&first, bad, 8, hipMemcpyDeviceToHost));
        if (first != ~0ull) {
            leann_set_error("%s: int8 rows need finite values; row %llu, column %llu is not finite", who, first / d, first % d);
            return LEANN_ERR_INVALID;
        }
        exps->resize(d);
        for (uint32_t j = 0; j < d; j++) {
            float a;
            memcpy(&a, &bits[j], 4);
            (*exps)[j] = (int8_t)i8_exponent(a);
        }
        return LEANN_OK;
    }
};

// h's exponents (host) and scales 2^-e_j (device, [g.ld], padding 1.0; g.norms); up: 2^e_j [g.ld] for the quantising kernel (may be null)
static int set_exponents(leann_backend *h, const int8_t *exps, DeviceBuf<float> *up) {
    const uint32_t d = h->g.d, ld = h->g.ld;
    std::vector<float> dn(ld, 1.0f), u(ld, 1.0f);
    for (uint32_t j = 0; j < d; j++) { dn[j] = i8_pow2(-exps[j]); u[j] = i8_pow2(exps[j]); }
    h->i8_exps.assign(exps, exps + d);
    if (h->store.norms.alloc(ld)) return LEANN_ERR_DEVICE;
    h->g.norms = h->store.norms;
    HIP_CHECK_RET(hipMemcpy(h->store.norms, dn.data(), (size_t)ld * 4, hipMemcpyHostToDevice));
    if (up) {
        if (up->alloc(ld)) return LEANN_ERR_DEVICE;
        HIP_CHECK_RET(hipMemcpy(*up, u.data(), (size_t)ld * 4, hipMemcpyHostToDevice));
    }
    return LEANN_OK;
}

static int launch_quantize(const float *d_src, size_t n, uint32_t d, size_t ld, uint32_t ldb, const float *up, const float *dn, int8_t *out,
                           float *deq) {
    if (n == 0) return LEANN_OK;
    const uint64_t items = (uint64_t)n * (ldb >> 2);
    const unsigned grid = (unsigned)std::min<uint64_t>((items + 255) / 256, 1u << 20);
    hipLaunchKernelGGL(quantize_rows_i8_kernel, dim3(grid), dim3(256), 0, nullptr, d_src, (uint64_t)n, d, (uint32_t)ld, ldb, up, dn, out, deq);
    HIP_CHECK_RET(hipGetLastError());
    HIP_CHECK_RET(hipDeviceSynchronize()); // null-stream work; searches run on non-blocking streams that do not wait for it
    return LEANN_OK;
}

// the store of h (h->g.n / d set), zero filled; h owns it from here on
static int alloc_store(leann_backend *h) {
    const uint32_t ldb = i8_store_ld(h->g.d);
    const size_t bytes = std::max<size_t>((size_t)h->g.n * ldb, 128);
    DeviceBuf<unsigned char> store;
    if (int rc = store.alloc(bytes)) return rc;
    HIP_CHECK_RET(hipMemset(store, 0, bytes));
    leann_internal_own_rows(h, std::move(store)); // (the handle is new, or borrowed the f32 rows it was built on until here)
    h->g.row_bytes = ldb;
    h->g.feat_h = 0;
    h->row_type = LEANN_ROWS_I8;
    return LEANN_OK;
}

// Quantise f32 device rows [n x ld_src]: *exps empty -> the column pass fills it (LEANN_ERR_INVALID naming the first non-finite
// element), else the given exponents are used; store: where the codes go (may be null); write_back: Xq over d_rows.  The
// scale arrays are sized to the source pitch: the kernels read them in groups of four columns up to that pitch.
int leann_internal_i8_quantize_device(const char *who, float *d_rows, size_t n, uint32_t d, size_t ld_src, std::vector<int8_t> *exps, int8_t *store,
                                      bool write_back) {
    if ((ld_src & 3) || ld_src < d || (n && !d_rows)) { leann_set_error("int8 rows: invalid source rows (ld %zu)", ld_src); return LEANN_ERR_INVALID; }
    if (exps->empty()) {
        ColumnPass cp;
        if (int rc = cp.begin(d, (uint32_t)ld_src)) return rc;
        if (int rc = cp.add(d_rows, n, 0)) return rc;
        if (int rc = cp.finish(who, exps)) return rc;
    }
    if (!store && !write_back) return LEANN_OK;
    std::vector<float> u(ld_src, 1.0f), v(ld_src, 1.0f);
    for (uint32_t j = 0; j < d; j++) { u[j] = i8_pow2((*exps)[j]); v[j] = i8_pow2(-(*exps)[j]); }
    DeviceBuf<float> up, dn;
    if (up.alloc(ld_src) || dn.alloc(ld_src)) return LEANN_ERR_DEVICE;
    HIP_CHECK_RET(hipMemcpy(up, u.data(), ld_src * 4, hipMemcpyHostToDevice));
    HIP_CHECK_RET(hipMemcpy(dn, v.data(), ld_src * 4, hipMemcpyHostToDevice));
    return launch_quantize(d_rows, n, d, ld_src, i8_store_ld(d), up, dn, store, write_back ? d_rows : nullptr);
}

int leann_internal_i8_adopt_device(leann_backend *h, const float *d_src, size_t ld_src, const char *who) {
    std::vector<int8_t> exps = h->i8_exps; // (a device build has run the column pass already: quantising Xq again gives the same codes)
    if (int rc = leann_internal_i8_quantize_device(who, const_cast<float *>(d_src), h->g.n, h->g.d, ld_src, &exps, nullptr, false)) return rc;
    if (int rc = set_exponents(h, exps.data(), nullptr)) return rc;
    if (int rc = alloc_store(h)) return rc;
    return leann_internal_i8_quantize_device(who, const_cast<float *>(d_src), h->g.n, h->g.d, ld_src, &exps, (int8_t *)h->g.X, false);
}

int leann_internal_i8_adopt_host(leann_backend *h, const float *f32_rows, const int8_t *codes, const int8_t *exps) {
    const size_t n = h->g.n, d = h->g.d;
    if (n && !f32_rows && !codes) { leann_set_error("int8 rows: no rows given"); return LEANN_ERR_INVALID; }
    if (codes && !exps) { leann_set_error("int8 rows: codes without their column exponents"); return LEANN_ERR_INVALID; }
    const uint32_t ldb = i8_store_ld((uint32_t)d);
    if (codes) { // an index file's rows: permuted on the host, slab by slab
        if (int rc = set_exponents(h, exps, nullptr)) return rc;
        if (int rc = alloc_store(h)) return rc;
        int8_t *store = (int8_t *)h->g.X;
        const size_t slab = std::max<size_t>(1, ((size_t)64 << 20) / ldb);
        std::vector<int8_t> buf(std::min(slab, std::max<size_t>(n, 1)) * ldb, (int8_t)0);
        for (size_t r0 = 0; r0 < n; r0 += slab) {
            const size_t m = std::min(slab, n - r0);
            for (size_t i = 0; i < m; i++)
                for (size_t j = 0; j < d; j++) buf[i * ldb + i8_row_pos((uint32_t)j, ldb)] = codes[(r0 + i) * d + j];
            HIP_CHECK_RET(hipMemcpy(store + r0 * ldb, buf.data(), m * ldb, hipMemcpyHostToDevice));
        }
        return LEANN_OK;
    }
    // f32 host rows: through a transient device slab, twice when they do not fit one — the column pass over all rows comes before the
    // first code — and quantised by the same kernel as every other way in
    const size_t ld = (d + 3) & ~(size_t)3, slab = std::max<size_t>(1, ((size_t)256 << 20) / (ld * 4));
    DeviceBuf<float> stage;
    if (int rc = stage.alloc(std::max<size_t>(std::min(slab, n) * ld, 4))) return rc;
    auto upload = [&](size_t r0, size_t m) {
        if (leann_internal_stage_rows(stage, ld, f32_rows + r0 * d, d, d, m, true) == hipSuccess) return (int)LEANN_OK;
        leann_set_error("int8 rows: upload of the rows failed: %s", hipGetErrorString(hipGetLastError()));
        return (int)LEANN_ERR_DEVICE;
    };
    ColumnPass cp;
    std::vector<int8_t> e;
    if (int rc = cp.begin((uint32_t)d, (uint32_t)ld)) return rc;
    for (size_t r0 = 0; r0 < n; r0 += slab) {
        const size_t m = std::min(slab, n - r0);
        if (int rc = upload(r0, m)) return rc;
        if (int rc = cp.add(stage, m, r0)) return rc;
        HIP_CHECK_RET(hipDeviceSynchronize()); // the next upload overwrites the slab
    }
    if (int rc = cp.finish("leann_backend_from_arrays_rows", &e)) return rc;
    DeviceBuf<float> up;
    if (int rc = set_exponents(h, e.data(), &up)) return rc;
    if (int rc = alloc_store(h)) return rc;
    int8_t *store = (int8_t *)h->g.X;
    for (size_t r0 = 0; r0 < n; r0 += slab) {
        const size_t m = std::min(slab, n - r0);
        if (n > slab)
            if (int rc = upload(r0, m)) return rc; // (one slab: it is still staged)
        if (int rc = launch_quantize(stage, m, (uint32_t)d, ld, ldb, up, h->g.norms, store + r0 * ldb, nullptr)) return rc;
    }
    return LEANN_OK;
}

int leann_internal_i8_to_host(const leann_backend *h, size_t r0, size_t rows, int8_t *out) {
    if (!leann_internal_i8(h) || r0 + rows > h->g.n) { leann_set_error("int8 rows: no such rows"); return LEANN_ERR_INVALID; }
    if (rows == 0) return LEANN_OK;
    const size_t d = h->g.d;
    const uint32_t ldb = h->g.row_bytes;
    const size_t slab = std::max<size_t>(1, ((size_t)64 << 20) / ldb);
    std::vector<int8_t> buf(std::min(slab, rows) * ldb);
    for (size_t s0 = 0; s0 < rows; s0 += slab) {
        const size_t m = std::min(slab, rows - s0);
        HIP_CHECK_RET(hipMemcpy(buf.data(), (const int8_t *)h->g.X + (r0 + s0) * ldb, m * ldb, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < m; i++)
            for (size_t j = 0; j < d; j++) out[(s0 + i) * d + j] = buf[i * ldb + i8_row_pos((uint32_t)j, ldb)];
    }
    return LEANN_OK;
}

int leann_internal_i8_carry_exponents(const leann_backend *src, leann_backend *dst) { return set_exponents(dst, src->i8_exps.data(), nullptr); }

const char *leann_internal_i8_check_file_rows(const int8_t *exps, const int8_t *codes, size_t n, size_t d) {
    for (size_t j = 0; j < d; j++)
        if (exps[j] > LEANN_I8_EXP_MAX || exps[j] < -LEANN_I8_EXP_MAX) return "int8 rows: a column exponent outside [-32, 32]";
    for (size_t i = 0; i < n * d; i++)
        if (codes[i] == -128) return "int8 rows: the code -128, which no quantised row holds";
    return nullptr;
}

// ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
extern "C" int leann_quantize_i8(const float *in, size_t n, size_t d, int8_t *exps, int8_t *codes) {
    if (d == 0 || !exps || (n && (!in || !codes))) { leann_set_error("leann_quantize_i8: null argument or no columns"); return LEANN_ERR_INVALID; }
    try {
        std::vector<float> amax(d, 0.f);
        for (size_t i = 0; i < n; i++)
            for (size_t j = 0; j < d; j++) {
                const float a = fabsf(in[i * d + j]);
                if (!(a <= 3.402823466e38f)) { // NaN or infinity
                    leann_set_error("leann_quantize_i8: int8 rows need finite values; row %zu, column %zu is not finite", i, j);
                    return LEANN_ERR_INVALID;
                }
                if (a > amax[j]) amax[j] = a;
            }
        std::vector<float> up(d);
        for (size_t j = 0; j < d; j++) { exps[j] = (int8_t)i8_exponent(amax[j]); up[j] = i8_pow2(exps[j]); }
        for (size_t i = 0; i < n; i++)
            for (size_t j = 0; j < d; j++) codes[i * d + j] = i8_code(in[i * d + j], up[j]);
        return LEANN_OK;
    } catch (const std::exception &e) {
        leann_set_error("leann_quantize_i8: %s", e.what());
        return LEANN_ERR_IO;
    }
}

extern "C" int leann_backend_rows_export_i8(const leann_backend *h, int8_t *exps, int8_t *rows) {
    if (!h || !exps || !rows) { leann_set_error("leann_backend_rows_export_i8: null argument"); return LEANN_ERR_INVALID; }
    if (h->sharded || !leann_internal_i8(h)) {
        leann_set_error("leann_backend_rows_export_i8: the handle stores no int8 rows (a composite handle: export its shards)");
        return LEANN_ERR_UNSUPPORTED;
    }
    try {
        HIP_CHECK_RET(hipSetDevice(h->device));
        HIP_CHECK_RET(hipDeviceSynchronize());
        memcpy(exps, h->i8_exps.data(), h->g.d);
        return leann_internal_i8_to_host(h, 0, h->g.n, rows);
    } catch (const std::exception &e) {
        leann_set_error("leann_backend_rows_export_i8: %s", e.what());
        return LEANN_ERR_IO;
    }
}
