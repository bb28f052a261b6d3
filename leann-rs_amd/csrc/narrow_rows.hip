// narrow_rows.hip — the row store of every narrow row type (narrow_rows.h: bf16, int8) and the entry points that make such handles:
// from arrays, by a device build on the narrowed rows, and from an f32 handle (leann_backend_to_rows).  Host code only, no kernel:
// the encode kernels sit beside their types' descriptions (rows_bf16.hip, rows_i8.hip), the search kernels in search_bf16.hip and
// search_i8.hip.  The element size is a number here, never a C type.
#include "common.cuh"
#include "internal.h"

#include <algorithm>

const NarrowRows *leann_internal_narrow(int row_type) {
    for (const NarrowRows *t : {leann_internal_bf16_rows(), leann_internal_i8_rows()})
        if (t->row_type == row_type) return t;
    return nullptr;
}
const NarrowRows *leann_internal_narrow_of_version(uint32_t file_version) {
    for (const NarrowRows *t : {leann_internal_bf16_rows(), leann_internal_i8_rows()})
        if (t->file_version == file_version) return t;
    return nullptr;
}

// The store of h (h->g.n / d set); h owns it from here on.  Not zero filled: every way in writes every byte of every row, padding
// included — the encode kernels store whole rows, an index file's rows go up as whole rows from a zeroed slab — and the 128 bytes of
// an empty index are never read.
static int alloc_store(leann_backend *h, const NarrowRows *t) {
    const uint32_t pitch = t->store_pitch(h->g.d);
    DeviceBuf<unsigned char> store;
    if (int rc = store.alloc(std::max<size_t>((size_t)h->g.n * pitch, 128))) return rc;
    leann_internal_own_rows(h, std::move(store)); // (the handle is new, or borrowed the f32 rows it was built on until here)
    h->g.row_bytes = pitch;
    h->g.feat_h = 0;
    h->row_type = t->row_type;
    return LEANN_OK;
}

// byte k of a row in element order sits at byte at[k] of its store row
static std::vector<uint32_t> byte_positions(const NarrowRows *t, size_t d, uint32_t pitch) {
    const uint32_t eb = t->elem_bytes;
    std::vector<uint32_t> at(d * eb);
    for (size_t j = 0; j < d; j++)
        for (uint32_t b = 0; b < eb; b++) at[j * eb + b] = t->pos((uint32_t)j, pitch / eb) * eb + b;
    return at;
}

// an index file's rows, in element order: permuted on the host and copied up in slabs of 64 MiB of store rows
static int upload_file_rows(leann_backend *h, const NarrowRows *t, const unsigned char *rows) {
    const size_t n = h->g.n, pitch = h->g.row_bytes, row_b = (size_t)h->g.d * t->elem_bytes, slab = std::max<size_t>(1, ((size_t)64 << 20) / pitch);
    const std::vector<uint32_t> at = byte_positions(t, h->g.d, (uint32_t)pitch);
    std::vector<unsigned char> buf(std::min(slab, n) * pitch, 0);
    for (size_t r0 = 0; r0 < n; r0 += slab) {
        const size_t m = std::min(slab, n - r0);
        for (size_t i = 0; i < m; i++)
            for (size_t k = 0; k < row_b; k++) buf[i * pitch + at[k]] = rows[(r0 + i) * row_b + k];
        HIP_CHECK_RET(hipMemcpy(h->store.rows + r0 * pitch, buf.data(), m * pitch, hipMemcpyHostToDevice));
    }
    return LEANN_OK;
}

int leann_internal_narrow_to_host(const leann_backend *h, size_t r0, size_t rows, void *out) {
    const NarrowRows *t = leann_internal_narrow(h->row_type);
    if (!t || r0 + rows > h->g.n) { leann_set_error("%s rows: no such rows", leann_internal_row_name(h)); return LEANN_ERR_INVALID; }
    if (rows == 0) return LEANN_OK;
    const size_t pitch = h->g.row_bytes, row_b = (size_t)h->g.d * t->elem_bytes, slab = std::max<size_t>(1, ((size_t)64 << 20) / pitch);
    const std::vector<uint32_t> at = byte_positions(t, h->g.d, (uint32_t)pitch);
    std::vector<unsigned char> buf(std::min(slab, rows) * pitch);
    for (size_t s0 = 0; s0 < rows; s0 += slab) {
        const size_t m = std::min(slab, rows - s0);
        HIP_CHECK_RET(hipMemcpy(buf.data(), h->store.rows.p + (r0 + s0) * pitch, m * pitch, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < m; i++)
            for (size_t k = 0; k < row_b; k++) static_cast<unsigned char *>(out)[(s0 + i) * row_b + k] = buf[i * pitch + at[k]];
    }
    return LEANN_OK;
}

int leann_internal_narrow_adopt(leann_backend *h, const NarrowRows *t, const float *host_f32, const NarrowSource &src, const char *who) {
    const size_t n = h->g.n;
    const uint32_t d = h->g.d;
    if (n && !host_f32 && !src.file_rows && !src.d_f32) { leann_set_error("%s rows: no rows given", t->name); return LEANN_ERR_INVALID; }
    if (src.d_f32 && ((src.d_ld & 3) || src.d_ld < d)) { leann_set_error("%s rows: invalid source rows (ld %zu)", t->name, src.d_ld); return LEANN_ERR_INVALID; }
    // The f32 rows as slabs on the device.  Device rows are one slab.  Host rows pass through a transient slab of at most 256 MiB; a
    // second pass uploads them again only when there is more than one slab (a single one is still staged).
    const size_t ld = src.d_f32 ? src.d_ld : (d + 3) & ~(size_t)3;
    const size_t slab = src.d_f32 ? std::max<size_t>(n, 1) : std::max<size_t>(1, ((size_t)256 << 20) / (ld * 4));
    DeviceBuf<float> stage;
    size_t staged = ~(size_t)0; // the first row of the slab `stage` holds
    const SlabLoop each_slab = [&](const SlabFn &fn) -> int {
        for (size_t r0 = 0; r0 < n; r0 += slab) {
            const size_t m = std::min(slab, n - r0);
            float *rows = const_cast<float *>(src.d_f32); // (read only: nothing here asks for the write-back)
            if (!rows) {
                if (!stage.p)
                    if (int rc = stage.alloc(std::min(slab, n) * ld)) return rc;
                if (staged != r0 && leann_internal_stage_rows(stage, ld, host_f32 + r0 * d, d, d, m, true) != hipSuccess) {
                    leann_set_error("%s rows: upload of the rows failed: %s", t->name, hipGetErrorString(hipGetLastError()));
                    return LEANN_ERR_DEVICE;
                }
                staged = r0;
                rows = stage;
            }
            if (int rc = fn(rows, m, r0)) return rc;
            HIP_CHECK_RET(hipDeviceSynchronize()); // the next upload overwrites the slab
        }
        return LEANN_OK;
    };
    if (t->fit) { // int8: the column exponents — an index file's, a device build's, or from a pass over all the rows — and their scales
        if (src.exps) h->i8_exps.assign(src.exps, src.exps + d);
        if (h->i8_exps.empty())
            if (int rc = t->fit(who, d, (uint32_t)ld, each_slab, &h->i8_exps)) return rc;
        if (int rc = leann_internal_i8_bind_scales(h)) return rc;
    }
    if (int rc = alloc_store(h, t)) return rc;
    if (n == 0) return LEANN_OK;
    if (src.file_rows) return upload_file_rows(h, t, static_cast<const unsigned char *>(src.file_rows));
    return each_slab([&](float *rows, size_t m, size_t r0) {
        return t->encode(rows, m, d, ld, h->i8_exps.data(), h->store.rows.p + r0 * (size_t)h->g.row_bytes, false);
    });
}

// ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
static int check_row_type(const char *who, int row_type) {
    if (row_type == LEANN_ROWS_F32 || leann_internal_narrow(row_type)) return LEANN_OK;
    leann_set_error("%s: unknown row type %d (LEANN_ROWS_F32 = 0, LEANN_ROWS_BF16 = 1 or LEANN_ROWS_I8 = 4)", who, row_type);
    return LEANN_ERR_INVALID;
}

extern "C" int leann_backend_row_type(const leann_backend *h) {
    if (!h) return -1;
    if (h->sharded) h = leann_internal_sharded_shard(h->sharded, 0);
    if (!h) return -1;
    return h->g.feat_h ? LEANN_ROWS_FEATURES : h->row_type;
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
    const char *const who = "leann_backend_build_device_rows";
    if (!out) { leann_set_error("%s: null output", who); return LEANN_ERR_INVALID; }
    *out = nullptr;
    if (int rc = check_row_type(who, row_type)) return rc;
    if (row_type == LEANN_ROWS_F32) // the existing call (rows borrowed, as with take_copy = 0)
        return leann_backend_build_device(backend, d_vectors, n, dims, ld, graph_degree, complexity, device, key_offset, 0, out);
    if ((n && !d_vectors) || dims == 0 || dims > 4096 || ld < dims || (ld & 3) || n >= (1ull << 31)) {
        leann_set_error("%s: invalid arguments (n=%zu dims=%zu ld=%zu)", who, n, dims, ld);
        return LEANN_ERR_INVALID;
    }
    if (int rc = leann_internal_check_build_args(backend, graph_degree, complexity)) return rc;
    if (int rc = leann_internal_check_device(device)) return rc;
    HIP_CHECK_RET(hipSetDevice(device));
    float *rows = d_vectors;
    DeviceBuf<float> copy;
    if (!may_overwrite && n) { // the caller's rows stay as they are: narrow a transient copy
        if (copy.alloc(n * ld) || hipMemcpy(copy, d_vectors, n * ld * 4, hipMemcpyDeviceToDevice) != hipSuccess) {
            leann_set_error("%s: copying %zu rows failed: %s", who, n, hipGetErrorString(hipGetLastError()));
            return LEANN_ERR_DEVICE;
        }
        rows = copy;
    }
    // X <- the widened narrow rows in place; the existing builder, unchanged, on those rows (borrowed); then the store — narrowing the
    // widened rows gives the narrow rows again — replaces them.  (int8: behind the column pass, which refuses a non-finite element
    // before any graph work; the exponents are kept for the store.)
    const NarrowRows *const t = leann_internal_narrow(row_type);
    std::vector<int8_t> exps;
    int rc = t->fit ? t->fit(who, (uint32_t)dims, (uint32_t)ld, [&](const SlabFn &fn) { return n ? fn(rows, n, 0) : (int)LEANN_OK; }, &exps) : (int)LEANN_OK;
    if (rc == LEANN_OK) rc = t->encode(rows, n, (uint32_t)dims, ld, exps.data(), nullptr, true);
    leann_backend *h = nullptr;
    // (no split planes are cut for the transient f32 rows: device memory peaks at these rows + the store, as the header promises)
    if (rc == LEANN_OK) rc = leann_internal_build_device_no_planes(backend, rows, n, dims, ld, graph_degree, complexity, device, key_offset, &h);
    if (rc == LEANN_OK) {
        std::lock_guard<std::mutex> lk(h->mu);
        h->row_screen.store(0);
        h->g.X = nullptr;
        h->g.ld = (uint32_t)((dims + 3) & ~(size_t)3); // the store's own geometry: the kernel choice must not depend on the caller's pitch
        h->i8_exps = exps;
        rc = leann_internal_narrow_adopt(h, t, nullptr, NarrowSource{nullptr, nullptr, rows, ld}, who);
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
    const NarrowRows *const t = leann_internal_narrow(row_type);
    if (leann_internal_narrow_rows(hc) || !t) {
        leann_set_error("leann_backend_to_rows: only f32 -> bf16 and f32 -> int8 are supported (%s -> %s asked for); rebuild from the f32 rows for anything else",
                        leann_internal_row_name(hc), t ? t->name : "f32");
        return LEANN_ERR_UNSUPPORTED;
    }
    try {
        const size_t n = hc->g.n;
        std::vector<uint8_t> levels(std::max<size_t>(n, 1));
        std::vector<uint32_t> uo(std::max<size_t>(n, 1)), a0(std::max<size_t>(n * hc->g.M0, 1)), aU(std::max<size_t>(hc->n_upper_lists * hc->g.M, 1));
        if (int rc = leann_backend_graph_export(hc, levels.data(), uo.data(), a0.data(), aU.data(), nullptr)) return rc; // (selects h's device)
        leann_backend *h = nullptr;
        const NarrowSource src{nullptr, nullptr, n ? hc->g.X : nullptr, hc->g.ld};
        int rc = leann_internal_from_host(hc->kind, n, hc->g.d, hc->g.M, hc->g.M0, hc->g.max_level, hc->g.entry, levels.data(), uo.data(), a0.data(),
                                          aU.data(), hc->n_upper_lists, nullptr, nullptr, 0, 0, nullptr, hc->device, hc->key_offset, &h, row_type, &src);
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

// the raw export: the store rows in element order, behind the exponents of a type that has them
static int export_rows(const char *who, int row_type, const leann_backend *h, int8_t *exps, void *rows) {
    const NarrowRows *const t = leann_internal_narrow(row_type);
    if (!h || !rows || (t->fit && !exps)) { leann_set_error("%s: null argument", who); return LEANN_ERR_INVALID; }
    if (h->sharded || h->row_type != row_type) {
        leann_set_error("%s: the handle stores no %s rows (a composite handle: export its shards)", who, t->name);
        return LEANN_ERR_UNSUPPORTED;
    }
    try {
        HIP_CHECK_RET(hipSetDevice(h->device));
        HIP_CHECK_RET(hipDeviceSynchronize());
        if (exps) memcpy(exps, h->i8_exps.data(), h->g.d);
        return leann_internal_narrow_to_host(h, 0, h->g.n, rows);
    } catch (const std::exception &e) {
        leann_set_error("%s: %s", who, e.what());
        return LEANN_ERR_IO;
    }
}
extern "C" int leann_backend_rows_export_bf16(const leann_backend *h, uint16_t *out) {
    return export_rows("leann_backend_rows_export_bf16", LEANN_ROWS_BF16, h, nullptr, out);
}
extern "C" int leann_backend_rows_export_i8(const leann_backend *h, int8_t *exps, int8_t *rows) {
    return export_rows("leann_backend_rows_export_i8", LEANN_ROWS_I8, h, exps, rows);
}
