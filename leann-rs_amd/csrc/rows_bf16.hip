// rows_bf16.hip — graph indexes whose rows are bf16 (LEANN_ROWS_BF16, include/leann_backend.h; DESIGN.md "bf16 rows").
//
// Definition: with r = f32 -> bf16 round to nearest even (bf16.h) and w = the exact widening b << 16, a bf16 index over rows X is
// the f32 index over w(r(X)) with the same graph, bit for bit.  The search kernels are search_bf16.hip's; this file holds the row
// store — rounding on the device, the way in from host rows and index files, the way out — and the entry points that make such a
// handle: from arrays, by a device build on the rounded rows, and from an f32 handle (leann_backend_to_rows).  The same entry points
// make int8 handles (LEANN_ROWS_I8): their row store is rows_i8.hip's.
//
// Device layout: [n x ldb] u16, ldb = dims rounded up to 64 elements, zero padded — a row is whole, aligned 128-B lines (768-d: 12) —
// with the elements in rs_plane_pos order (row_screen.h): lane l of a wave finds its eight halves of a 512-element block in one
// 16-byte load.  g.X names the store, g.row_bytes = 2 ldb; g.ld keeps the f32 meaning (dims rounded up to 4) and selects the kernel.
// Files and exports are in plain element order.
#include "common.cuh"
#include "internal.h"
#include "bf16.h"
#include "row_screen.h"

#include <algorithm>
#include <new>
#include <vector>

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

// the store of h (h->g.n / d set), zero filled; h owns it from here on
static int alloc_store(leann_backend *h) {
    const uint32_t ldb = store_ld(h->g.d);
    const size_t bytes = std::max<size_t>((size_t)h->g.n * ldb * 2, 128);
    DeviceBuf<unsigned char> store;
    if (int rc = store.alloc(bytes)) return rc;
    leann_internal_own_rows(h, std::move(store)); // (the handle is new, or borrowed the f32 rows it was built on until here)
    h->g.row_bytes = ldb * 2;
    h->g.feat_h = 0;
    h->row_type = LEANN_ROWS_BF16;
    return LEANN_OK;
}

int leann_internal_bf16_adopt_device(leann_backend *h, const float *d_src, size_t ld_src) {
    if ((ld_src & 3) || ld_src < h->g.d || (h->g.n && !d_src)) { leann_set_error("bf16 rows: invalid source rows (ld %zu)", ld_src); return LEANN_ERR_INVALID; }
    if (int rc = alloc_store(h)) return rc;
    return launch_round(d_src, h->g.n, h->g.d, ld_src, h->g.row_bytes >> 1, (uint16_t *)h->g.X, nullptr);
}

int leann_internal_bf16_adopt_host(leann_backend *h, const float *f32_rows, const uint16_t *bf16_rows) {
    const size_t n = h->g.n, d = h->g.d;
    if (n && !f32_rows && !bf16_rows) { leann_set_error("bf16 rows: no rows given"); return LEANN_ERR_INVALID; }
    if (int rc = alloc_store(h)) return rc;
    if (n == 0) return LEANN_OK;
    const uint32_t ldb = h->g.row_bytes >> 1;
    uint16_t *store = (uint16_t *)h->g.X;
    if (bf16_rows) { // an index file's rows: permuted on the host, slab by slab
        const size_t slab = std::max<size_t>(1, ((size_t)64 << 20) / (ldb * 2));
        std::vector<uint16_t> buf(std::min(slab, n) * ldb, (uint16_t)0);
        for (size_t r0 = 0; r0 < n; r0 += slab) {
            const size_t m = std::min(slab, n - r0);
            for (size_t i = 0; i < m; i++)
                for (size_t j = 0; j < d; j++) buf[i * ldb + rs_plane_pos((uint32_t)j, ldb)] = bf16_rows[(r0 + i) * d + j];
            HIP_CHECK_RET(hipMemcpy(store + r0 * ldb, buf.data(), m * ldb * 2, hipMemcpyHostToDevice));
        }
        return LEANN_OK;
    }
    // f32 host rows: through a transient device slab, rounded by the same kernel as every other way in
    const size_t ld = (d + 3) & ~(size_t)3, slab = std::max<size_t>(1, ((size_t)256 << 20) / (ld * 4));
    DeviceBuf<float> stage;
    int rc = stage.alloc(std::min(slab, n) * ld);
    for (size_t r0 = 0; rc == LEANN_OK && r0 < n; r0 += slab) {
        const size_t m = std::min(slab, n - r0);
        if (leann_internal_stage_rows(stage, ld, f32_rows + r0 * d, d, d, m, true) != hipSuccess) {
            leann_set_error("bf16 rows: upload of the rows failed: %s", hipGetErrorString(hipGetLastError()));
            rc = LEANN_ERR_DEVICE;
            break;
        }
        rc = launch_round(stage, m, (uint32_t)d, ld, ldb, store + r0 * ldb, nullptr);
    }
    return rc;
}

int leann_internal_bf16_to_host(const leann_backend *h, size_t r0, size_t rows, uint16_t *out) {
    if (!leann_internal_bf16(h) || r0 + rows > h->g.n) { leann_set_error("bf16 rows: no such rows"); return LEANN_ERR_INVALID; }
    if (rows == 0) return LEANN_OK;
    const size_t d = h->g.d;
    const uint32_t ldb = h->g.row_bytes >> 1;
    const size_t slab = std::max<size_t>(1, ((size_t)64 << 20) / (ldb * 2));
    std::vector<uint16_t> buf(std::min(slab, rows) * ldb);
    for (size_t s0 = 0; s0 < rows; s0 += slab) {
        const size_t m = std::min(slab, rows - s0);
        HIP_CHECK_RET(hipMemcpy(buf.data(), (const uint16_t *)h->g.X + (r0 + s0) * ldb, m * ldb * 2, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < m; i++)
            for (size_t j = 0; j < d; j++) out[(s0 + i) * d + j] = buf[i * ldb + rs_plane_pos((uint32_t)j, ldb)];
    }
    return LEANN_OK;
}

// ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
static int check_row_type(const char *who, int row_type) {
    if (row_type == LEANN_ROWS_F32 || row_type == LEANN_ROWS_BF16 || row_type == LEANN_ROWS_I8) return LEANN_OK;
    leann_set_error("%s: unknown row type %d (LEANN_ROWS_F32 = 0, LEANN_ROWS_BF16 = 1 or LEANN_ROWS_I8 = 4)", who, row_type);
    return LEANN_ERR_INVALID;
}

extern "C" int leann_backend_row_type(const leann_backend *h) {
    if (!h) return -1;
    if (h->sharded) h = leann_internal_sharded_shard(h->sharded, 0);
    if (!h) return -1;
    return h->g.feat_h ? LEANN_ROWS_FEATURES : h->row_type;
}

extern "C" int leann_round_bf16(const float *in, size_t n, uint16_t *out) {
    if (n && (!in || !out)) { leann_set_error("leann_round_bf16: null argument"); return LEANN_ERR_INVALID; }
    for (size_t i = 0; i < n; i++) out[i] = f32_to_bf16_rne(in[i]);
    return LEANN_OK;
}

extern "C" int leann_backend_from_arrays_rows(int backend, const float *vectors, size_t n, size_t dims, uint32_t M, uint32_t M0,
                                              uint32_t max_level, uint32_t entry, const uint8_t *levels, const uint32_t *upper_off,
                                              const uint32_t *adj0, const uint32_t *adjU, size_t n_upper_lists, int device,
                                              uint64_t key_offset, int row_type, leann_backend **out) {
    if (!out) { leann_set_error("leann_backend_from_arrays_rows: null output"); return LEANN_ERR_INVALID; }
    *out = nullptr;
    if (int rc = check_row_type("leann_backend_from_arrays_rows", row_type)) return rc;
    if (row_type == LEANN_ROWS_F32)
        return leann_backend_from_arrays(backend, vectors, n, dims, M, M0, max_level, entry, levels, upper_off, adj0, adjU, n_upper_lists, device,
                                         key_offset, out);
    try {
        return leann_internal_from_host(backend, n, dims, M, M0, max_level, entry, levels, upper_off, adj0, adjU, n_upper_lists, vectors, nullptr,
                                        0, 0, nullptr, device, key_offset, out, row_type);
    } catch (const std::exception &e) {
        leann_set_error("leann_backend_from_arrays_rows: %s", e.what());
        return LEANN_ERR_IO;
    }
}

extern "C" int leann_backend_build_device_rows(int backend, float *d_vectors, size_t n, size_t dims, size_t ld, size_t graph_degree,
                                               size_t complexity, int device, uint64_t key_offset, int row_type, int may_overwrite,
                                               leann_backend **out) {
    if (!out) { leann_set_error("leann_backend_build_device_rows: null output"); return LEANN_ERR_INVALID; }
    *out = nullptr;
    if (int rc = check_row_type("leann_backend_build_device_rows", row_type)) return rc;
    if (row_type == LEANN_ROWS_F32) // the existing call (rows borrowed, as with take_copy = 0)
        return leann_backend_build_device(backend, d_vectors, n, dims, ld, graph_degree, complexity, device, key_offset, 0, out);
    if ((n && !d_vectors) || dims == 0 || dims > 4096 || ld < dims || (ld & 3) || n >= (1ull << 31)) {
        leann_set_error("leann_backend_build_device_rows: invalid arguments (n=%zu dims=%zu ld=%zu)", n, dims, ld);
        return LEANN_ERR_INVALID;
    }
    if (int rc = leann_internal_check_build_args(backend, graph_degree, complexity)) return rc;
    if (int rc = leann_internal_check_device(device)) return rc;
    HIP_CHECK_RET(hipSetDevice(device));
    float *rows = d_vectors;
    DeviceBuf<float> copy;
    if (!may_overwrite && n) { // the caller's rows stay as they are: round a transient copy
        if (copy.alloc(n * ld) || hipMemcpy(copy, d_vectors, n * ld * 4, hipMemcpyDeviceToDevice) != hipSuccess) {
            leann_set_error("leann_backend_build_device_rows: copying %zu rows failed: %s", n, hipGetErrorString(hipGetLastError()));
            return LEANN_ERR_DEVICE;
        }
        rows = copy;
    }
    // X <- w(r(X)) in place; the existing builder, unchanged, on those rows (borrowed); then the store — r(w(r(x))) = r(x) — replaces them
    // (int8: X <- Xq behind the column pass, which refuses a non-finite element before any graph work; the exponents are kept for the
    // store, and quantising Xq with them gives the codes again)
    const bool i8 = row_type == LEANN_ROWS_I8;
    std::vector<int8_t> exps;
    int rc = i8 ? leann_internal_i8_quantize_device("leann_backend_build_device_rows", rows, n, (uint32_t)dims, ld, &exps, nullptr, true)
                : launch_round(rows, n, (uint32_t)dims, ld, store_ld((uint32_t)dims), nullptr, rows);
    leann_backend *h = nullptr;
    // (no split planes are cut for the transient f32 rows: device memory peaks at these rows + the store, as the header promises)
    if (rc == LEANN_OK) rc = leann_internal_build_device_no_planes(backend, rows, n, dims, ld, graph_degree, complexity, device, key_offset, &h);
    if (rc == LEANN_OK) {
        std::lock_guard<std::mutex> lk(h->mu);
        h->row_screen.store(0);
        h->g.X = nullptr;
        h->g.ld = (uint32_t)((dims + 3) & ~(size_t)3); // the store's own geometry: the kernel choice must not depend on the caller's pitch
        if (i8) h->i8_exps = exps;
        rc = i8 ? leann_internal_i8_adopt_device(h, rows, ld, "leann_backend_build_device_rows") : leann_internal_bf16_adopt_device(h, rows, ld);
    }
    copy.reset();
    if (rc) { if (h) leann_backend_close(h); return rc; }
    *out = h;
    return LEANN_OK;
}

extern "C" int leann_backend_build_rows(int backend, const float *vectors, size_t n, size_t dims, size_t graph_degree, size_t complexity,
                                        int row_type, const char *index_path_stem) {
    if (int rc = check_row_type("leann_backend_build_rows", row_type)) return rc;
    if (row_type == LEANN_ROWS_F32) return leann_backend_build(backend, vectors, n, dims, graph_degree, complexity, index_path_stem);
    if (!index_path_stem || (n && !vectors) || dims == 0 || dims > 4096) {
        leann_set_error("leann_backend_build_rows: invalid arguments");
        return LEANN_ERR_INVALID;
    }
    if (int rc = leann_internal_check_build_args(backend, graph_degree, complexity)) return rc;
    if (int rc = leann_internal_use_device0()) return rc;
    const size_t ld = (dims + 3) & ~(size_t)3;
    DeviceBuf<float> dX;
    if (dX.alloc(std::max<size_t>(n * ld, 4)) || leann_internal_stage_rows(dX, ld, vectors, dims, dims, n, true) != hipSuccess) {
        leann_set_error("leann_backend_build_rows: upload of %zu rows failed: %s", n, hipGetErrorString(hipGetLastError()));
        return LEANN_ERR_DEVICE;
    }
    leann_backend *h = nullptr;
    int rc = leann_backend_build_device_rows(backend, dX, n, dims, ld, graph_degree, complexity, 0, 0, row_type, 1, &h);
    dX.reset(); // the upload was this call's own copy: built on in place, not kept
    if (rc) return rc;
    rc = leann_backend_save(h, index_path_stem);
    leann_backend_close(h);
    return rc;
}

extern "C" int leann_backend_to_rows(const leann_backend *hc, int row_type, leann_backend **out) {
    if (!hc || !out) { leann_set_error("leann_backend_to_rows: null argument"); return LEANN_ERR_INVALID; }
    *out = nullptr;
    if (int rc = check_row_type("leann_backend_to_rows", row_type)) return rc;
    if (hc->sharded) {
        leann_set_error("leann_backend_to_rows: not available on a composite handle; convert each shard (leann_backend_shard), then leann_sharded_from_handles");
        return LEANN_ERR_UNSUPPORTED;
    }
    if (hc->g.feat_h) {
        leann_set_error("leann_backend_to_rows: a recompute-on index holds no vectors to convert");
        return LEANN_ERR_UNSUPPORTED;
    }
    if (leann_internal_narrow_rows(hc) || row_type == LEANN_ROWS_F32) {
        leann_set_error("leann_backend_to_rows: only f32 -> bf16 and f32 -> int8 are supported (%s -> %s asked for); rebuild from the f32 rows for anything else",
                        leann_internal_row_name(hc), row_type == LEANN_ROWS_BF16 ? "bf16" : row_type == LEANN_ROWS_I8 ? "int8" : "f32");
        return LEANN_ERR_UNSUPPORTED;
    }
    try {
        const size_t n = hc->g.n;
        std::vector<uint8_t> levels(std::max<size_t>(n, 1));
        std::vector<uint32_t> uo(std::max<size_t>(n, 1)), a0(std::max<size_t>(n * hc->g.M0, 1)), aU(std::max<size_t>(hc->n_upper_lists * hc->g.M, 1));
        if (int rc = leann_backend_graph_export(hc, levels.data(), uo.data(), a0.data(), aU.data(), nullptr)) return rc; // (selects h's device)
        leann_backend *h = nullptr;
        int rc = leann_internal_from_host(hc->kind, n, hc->g.d, hc->g.M, hc->g.M0, hc->g.max_level, hc->g.entry, levels.data(), uo.data(), a0.data(),
                                          aU.data(), hc->n_upper_lists, nullptr, nullptr, 0, 0, nullptr, hc->device, hc->key_offset, &h, row_type,
                                          nullptr, n ? hc->g.X : nullptr, hc->g.ld);
        if (rc) return rc;
        leann_internal_take_build_params(h, hc); // (the arrays went through from_host, which knows no source handle)
        rc = leann_internal_carry_removals(hc, h, n);
        if (rc) { leann_backend_close(h); return rc; }
        *out = h;
        return LEANN_OK;
    } catch (const std::exception &e) {
        leann_set_error("leann_backend_to_rows: %s", e.what());
        return LEANN_ERR_IO;
    }
}

extern "C" int leann_backend_rows_export_bf16(const leann_backend *h, uint16_t *out) {
    if (!h || !out) { leann_set_error("leann_backend_rows_export_bf16: null argument"); return LEANN_ERR_INVALID; }
    if (h->sharded || !leann_internal_bf16(h)) {
        leann_set_error("leann_backend_rows_export_bf16: the handle stores no bf16 rows (a composite handle: export its shards)");
        return LEANN_ERR_UNSUPPORTED;
    }
    try {
        HIP_CHECK_RET(hipSetDevice(h->device));
        HIP_CHECK_RET(hipDeviceSynchronize());
        return leann_internal_bf16_to_host(h, 0, h->g.n, out);
    } catch (const std::exception &e) {
        leann_set_error("leann_backend_rows_export_bf16: %s", e.what());
        return LEANN_ERR_IO;
    }
}
