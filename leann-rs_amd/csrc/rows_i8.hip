// rows_i8.hip — graph indexes whose rows are int8 codes with one power-of-two scale per column (LEANN_ROWS_I8,
// include/leann_backend.h; DESIGN.md "int8 rows").
//
// Definition (i8_rows.h): amax_j = max_i |x_ij|, e_j the largest integer in [-32, 32] with amax_j 2^e_j <= 127 (0 for a zero column),
// c_ij = clamp(rne(x_ij 2^e_j), -127, 127), Xq_ij = (float)c_ij 2^-e_j.  An int8 index over rows X is the f32 index over Xq with the
// same graph, bit for bit.  The search kernels are search_i8.hip's; the row store and the entry points that make such a handle are
// narrow_rows.hip's, shared with every narrow type.  This file holds what is int8's alone: the column reduction and the quantising
// kernel, the exponents and their scales, the type's description for that store (narrow_rows.h), the check of an index file's rows
// and the host quantiser leann_quantize_i8.
//
// Store row: ldb = dims rounded up to 128 bytes, zero padded — whole, aligned 128-B lines (768-d: 6) — with the elements in
// i8_row_pos order (i8_rows.h).  g.norms names the column scales 2^-e_j, f32 [g.ld], padding 1.0.  The exponents stay on the host
// (leann_backend::i8_exps).
#include "common.cuh"
#include "internal.h"
#include "i8_rows.h"

#include <algorithm>
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

int leann_internal_i8_bind_scales(leann_backend *h) {
    const uint32_t d = h->g.d, ld = h->g.ld;
    std::vector<float> dn(ld, 1.0f);
    for (uint32_t j = 0; j < d; j++) dn[j] = i8_pow2(-h->i8_exps[j]);
    if (h->store.norms.alloc(ld)) return LEANN_ERR_DEVICE;
    h->g.norms = h->store.norms;
    HIP_CHECK_RET(hipMemcpy(h->store.norms, dn.data(), (size_t)ld * 4, hipMemcpyHostToDevice));
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

// ---- the type's description for the shared store (narrow_rows.h) ---------------------------------------------------------------------
static uint32_t store_pitch(uint32_t d) { return i8_store_ld(d); }
static uint32_t store_pos(uint32_t j, uint32_t ldb) { return i8_row_pos(j, ldb); }
// the column pass over all rows comes before the first code: LEANN_ERR_INVALID naming the first non-finite element
static int fit(const char *who, uint32_t d, uint32_t ld, const SlabLoop &each_slab, std::vector<int8_t> *exps) {
    ColumnPass cp;
    if (int rc = cp.begin(d, ld)) return rc;
    if (int rc = each_slab([&](float *d_rows, size_t m, size_t row0) { return cp.add(d_rows, m, row0); })) return rc;
    return cp.finish(who, exps);
}
// The scale arrays are sized to the source pitch: the kernel reads them in groups of four columns up to that pitch.
static int encode(float *d_rows, size_t m, uint32_t d, size_t ld, const int8_t *exps, void *store, bool write_back) {
    if (m == 0 || (!store && !write_back)) return LEANN_OK;
    std::vector<float> u(ld, 1.0f), v(ld, 1.0f);
    for (uint32_t j = 0; j < d; j++) { u[j] = i8_pow2(exps[j]); v[j] = i8_pow2(-exps[j]); }
    DeviceBuf<float> up, dn;
    if (up.alloc(ld) || dn.alloc(ld)) return LEANN_ERR_DEVICE;
    HIP_CHECK_RET(hipMemcpy(up, u.data(), ld * 4, hipMemcpyHostToDevice));
    HIP_CHECK_RET(hipMemcpy(dn, v.data(), ld * 4, hipMemcpyHostToDevice));
    return launch_quantize(d_rows, m, d, ld, i8_store_ld(d), up, dn, (int8_t *)store, write_back ? d_rows : nullptr);
}
// Xq = code x 2^-e: exact
static void widen(const unsigned char *src, size_t count, size_t d, const int8_t *exps, unsigned char *dst) {
    for (size_t i = 0; i < count; i++) {
        const float x = (float)(int8_t)src[i] * ldexpf(1.0f, -exps[i % d]);
        memcpy(dst + 4 * i, &x, 4);
    }
}
const NarrowRows *leann_internal_i8_rows() { // (a function: a const object at namespace scope would be emitted into the device code too)
    static const NarrowRows t = {LEANN_ROWS_I8, "int8", 1, 4, store_pitch, store_pos, fit, encode, widen};
    return &t;
}

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
