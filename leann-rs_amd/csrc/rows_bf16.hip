// rows_bf16.hip — bf16 rows (LEANN_ROWS_BF16, include/leann_backend.h; DESIGN.md "bf16 rows"): what is this type's alone.
//
// Definition: with r = f32 -> bf16 round to nearest even (bf16.h) and w = the exact widening b << 16, a bf16 index over rows X is
// the f32 index over w(r(X)) with the same graph, bit for bit.  The search kernels are search_bf16.hip's; the row store and the entry
// points that make such a handle are narrow_rows.hip's, shared with every narrow type.  This file holds the rounding kernel, the
// type's description for that store (narrow_rows.h) and the host rounding leann_round_bf16.
//
// Store row: ldb = dims rounded up to 64 elements of u16, zero padded — whole, aligned 128-B lines (768-d: 12) — with the elements in
// rs_plane_pos order (row_screen.h): lane l of a wave finds its eight halves of a 512-element block in one 16-byte load.
#include "common.cuh"
#include "internal.h"
#include "bf16.h"
#include "row_screen.h"

#include <algorithm>

// one work item = four elements 4 i .. 4 i + 3 of a store row (contiguous in X and in the store).  out: the store (may be null);
// widened: w(r(x)) written back over X (may be null: leann_backend_build_device_rows builds on the rounded rows).
__global__ void __launch_bounds__(256) round_rows_bf16_kernel(const float *X, uint64_t n, uint32_t d, uint32_t ld, uint32_t ldb,
                                                              uint16_t *__restrict__ out, float *widened /* may be X itself */) {
    const uint32_t per_row = ldb >> 2;
    const uint64_t items = n * per_row;
    for (uint64_t it = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t row = it / per_row;
        const uint32_t j = (uint32_t)(it - row * per_row) << 2;
        uint16_t b[4] = {0, 0, 0, 0};
        if (j < ld) { // ld is a multiple of 4: the group is inside the row or padding
            const float4 v = *reinterpret_cast<const float4 *>(X + row * ld + j);
            b[0] = j + 0 < d ? f32_to_bf16_rne(v.x) : (uint16_t)0; // (elements past dims are padding: zero in the store whatever X holds)
            b[1] = j + 1 < d ? f32_to_bf16_rne(v.y) : (uint16_t)0;
            b[2] = j + 2 < d ? f32_to_bf16_rne(v.z) : (uint16_t)0;
            b[3] = j + 3 < d ? f32_to_bf16_rne(v.w) : (uint16_t)0;
            if (widened)
                *reinterpret_cast<uint4 *>(widened + row * ld + j) =
                    make_uint4((uint32_t)b[0] << 16, (uint32_t)b[1] << 16, (uint32_t)b[2] << 16, (uint32_t)b[3] << 16);
        }
        if (out)
            *reinterpret_cast<uint2 *>(out + (size_t)row * ldb + rs_plane_pos(j, ldb)) =
                make_uint2((uint32_t)b[0] | ((uint32_t)b[1] << 16), (uint32_t)b[2] | ((uint32_t)b[3] << 16));
    }
}

static uint32_t store_ld(uint32_t d) { return (d + 63u) & ~63u; }

static int launch_round(const float *d_src, size_t n, uint32_t d, size_t ld, uint32_t ldb, uint16_t *out, float *widened) {
    if (n == 0) return LEANN_OK;
    const uint64_t items = (uint64_t)n * (ldb >> 2);
    const unsigned grid = (unsigned)std::min<uint64_t>((items + 255) / 256, 1u << 20);
    hipLaunchKernelGGL(round_rows_bf16_kernel, dim3(grid), dim3(256), 0, nullptr, d_src, (uint64_t)n, d, (uint32_t)ld, ldb, out, widened);
    HIP_CHECK_RET(hipGetLastError());
    HIP_CHECK_RET(hipDeviceSynchronize()); // null-stream work; searches run on non-blocking streams that do not wait for it
    return LEANN_OK;
}

// ---- the type's description for the shared store (narrow_rows.h) ---------------------------------------------------------------------
static uint32_t store_pitch(uint32_t d) { return store_ld(d) * 2; }
static uint32_t store_pos(uint32_t j, uint32_t ldb) { return rs_plane_pos(j, ldb); }
static int encode(float *d_rows, size_t m, uint32_t d, size_t ld, const int8_t *, void *store, bool write_back) {
    return launch_round(d_rows, m, d, ld, store_ld(d), (uint16_t *)store, write_back ? d_rows : nullptr);
}
// w(rows): exact
static void widen(const unsigned char *src, size_t count, size_t, const int8_t *, unsigned char *dst) {
    for (size_t i = 0; i < count; i++) {
        uint16_t b;
        memcpy(&b, src + 2 * i, 2);
        const uint32_t w = (uint32_t)b << 16;
        memcpy(dst + 4 * i, &w, 4);
    }
}
const NarrowRows *leann_internal_bf16_rows() { // (a function: a const object at namespace scope would be emitted into the device code too)
    static const NarrowRows t = {LEANN_ROWS_BF16, "bf16", 2, 3, store_pitch, store_pos, nullptr, encode, widen};
    return &t;
}

extern "C" int leann_round_bf16(const float *in, size_t n, uint16_t *out) {
    if (n && (!in || !out)) { leann_set_error("leann_round_bf16: null argument"); return LEANN_ERR_INVALID; }
    for (size_t i = 0; i < n; i++) out[i] = f32_to_bf16_rne(in[i]);
    return LEANN_OK;
}
