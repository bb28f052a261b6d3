// handle.hip — making a leann_backend: the steps every way in shares, stated once (contracts: internal.h).  Host code only, no
// kernel.  A new way in starts here; build.hip, compact.hip, narrow_rows.hip, indexfile.hip and shard.hip keep only what is their own.
#include "common.cuh"
#include "internal.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

hipError_t leann_internal_stage_rows(float *dst, size_t dst_ld, const float *src, size_t src_ld, size_t dims, size_t rows, bool from_host) {
    if (rows == 0) return hipSuccess;
    const hipMemcpyKind kind = from_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    if (dst_ld == dims && src_ld == dims) return hipMemcpy(dst, src, rows * dims * 4, kind);
    if (dst_ld != dims)
        if (hipError_t e = hipMemset(dst, 0, rows * dst_ld * 4)) return e;
    return hipMemcpy2D(dst, dst_ld * 4, src, src_ld * 4, dims * 4, rows, kind);
}

int leann_internal_rows_from_file(const std::string &path, uint64_t byte_offset, size_t rows, size_t dims, int device, DeviceBuf<float> *out) {
    std::unique_ptr<FILE, int (*)(FILE *)> f(fopen(path.c_str(), "rb"), fclose);
    if (!f || fseeko(f.get(), (off_t)byte_offset, SEEK_SET) != 0) return LEANN_ERR_NOT_FOUND;
    if (int rc = leann_internal_check_device(device)) return rc;
    if (hipSetDevice(device) != hipSuccess) { leann_set_error("hipSetDevice(%d) failed", device); return LEANN_ERR_DEVICE; }
    const size_t ld = (dims + 3) & ~(size_t)3;
    if (int rc = out->alloc(std::max<size_t>(rows * ld, 4))) return rc;
    const size_t slab_rows = std::max<size_t>(1, ((size_t)256 << 20) / (dims * 4));
    std::vector<float> slab(std::min(slab_rows, std::max<size_t>(rows, 1)) * dims);
    for (size_t r0 = 0; r0 < rows; r0 += slab_rows) {
        const size_t m = std::min(slab_rows, rows - r0);
        if (fread(slab.data(), dims * 4, m, f.get()) != m ||
            leann_internal_stage_rows(out->p + r0 * ld, ld, slab.data(), dims, dims, m, true) != hipSuccess) {
            out->reset();
            return LEANN_ERR_IO;
        }
    }
    return LEANN_OK;
}

int leann_internal_rebuild_from_rows(int backend, DeviceBuf<float> &&rows, size_t n, size_t dims, int device, uint64_t key_offset,
                                     const std::string &cache_path, leann_backend **out) {
    // the reference's own build defaults are graph_degree 32, complexity 64 (src/cli/build.rs:78-83); a wider construction beam costs
    // seconds here.  Vamana needs R = 64 beyond ~1M rows.
    size_t degree = backend == LEANN_BACKEND_HNSW ? 32 : 64, complexity = 128;
    if (const char *e = getenv("LEANN_REBUILD_DEGREE")) degree = (size_t)atoi(e);
    if (const char *e = getenv("LEANN_REBUILD_COMPLEXITY")) complexity = (size_t)atoi(e);
    if (int rc = leann_backend_build_device(backend, rows, n, dims, (dims + 3) & ~(size_t)3, degree, complexity, device, key_offset, 0, out)) return rc;
    leann_internal_own_rows(*out, std::move(rows));
    if (leann_internal_save_to(*out, cache_path) != LEANN_OK) // read-only directory: serve from memory, rebuild again next time
        leann_log(LEANN_LOG_WARN, "could not cache the rebuilt graph as %s (%s); it will be rebuilt on the next open", cache_path.c_str(), leann_last_error());
    return LEANN_OK;
}

int leann_internal_use_device0() {
    int ndev = 0;
    leann_device_count(&ndev);
    if (ndev < 1) { leann_set_error("no HIP device visible. This library has no CPU fallback."); return LEANN_ERR_DEVICE; }
    HIP_CHECK_RET(hipSetDevice(0));
    return LEANN_OK;
}

HandlePtr leann_internal_new_like(const leann_backend *src) {
    HandlePtr h(new leann_backend());
    h->kind = src->kind;
    h->device = src->device;
    h->key_offset = src->key_offset;
    leann_internal_take_build_params(h.get(), src);
    h->row_type = src->row_type;
    h->g = src->g; // n, d, ld, M, M0, entry, max_level, feat_h, row_bytes
    h->g.X = nullptr; h->g.adj0 = nullptr; h->g.adjU = nullptr; h->g.upper_off = nullptr; h->g.norms = nullptr;
    return h;
}
void leann_internal_take_build_params(leann_backend *dst, const leann_backend *src) {
    dst->efc = src->efc;
    dst->alpha = src->alpha;
    dst->two_stage = src->two_stage;
    dst->nav_levels = src->nav_levels;
    dst->fixed_ef = src->fixed_ef;
}

int leann_internal_carry_removals(const leann_backend *src, leann_backend *dst, size_t n_new) {
    std::vector<uint8_t> removed;
    size_t n_removed = 0;
    {
        std::lock_guard<std::mutex> lk(const_cast<leann_backend *>(src)->mu); // (leann_backend_remove takes it)
        n_removed = src->n_removed;
        if (n_removed) removed = src->removed;
    }
    if (!n_removed) return LEANN_OK;
    removed.resize((n_new + 7) / 8, 0); // zero bits: the new rows are live
    return leann_internal_set_removed(dst, removed.data(), n_removed); // the live mask uploaded, n_pending counted on the device
}

uint64_t leann_internal_upper_offsets(const uint8_t *levels, size_t n, uint32_t *uo) {
    uint64_t nu = 0;
    for (size_t i = 0; i < n; i++) { uo[i] = (uint32_t)nu; nu += levels[i]; }
    return nu;
}

int leann_internal_alloc_graph_lists(leann_backend *h, uint64_t n_upper_lists) {
    const size_t nn = std::max<size_t>(h->g.n, 1), nu = std::max<uint64_t>(n_upper_lists, 1);
    GraphStore &st = h->store;
    if (st.adj0.alloc(nn * h->g.M0) || st.adjU.alloc(nu * h->g.M) || st.upper_off.alloc(nn) || (!st.levels.p && st.levels.alloc(nn))) return LEANN_ERR_DEVICE;
    h->g.adj0 = st.adj0; h->g.adjU = st.adjU; h->g.upper_off = st.upper_off;
    h->n_upper_lists = n_upper_lists;
    HIP_CHECK_RET(hipMemset(st.adjU, 0xFF, nu * h->g.M * 4));
    return LEANN_OK;
}

// ---- in-memory construction from host arrays ----------------------------------------------------------
// Every array is checked against n BEFORE anything is uploaded: the traversal kernel indexes rows by neighbour id, upper lists by
// upper_off[node] + level - 1 and trusts both (search.cuh), so one bad entry in an index file would be an out-of-bounds read on the GPU.
static const char *validate_graph(size_t n, uint32_t M, uint32_t M0, uint32_t max_level, uint32_t entry, const uint8_t *levels,
                                  const uint32_t *upper_off, const uint32_t *adj0, const uint32_t *adjU, size_t n_upper_lists) {
    if (M == 0 || M0 == 0 || M > 128 || M0 > 128) return "graph degree outside [1, 128]";
    if (max_level > 15) return "max_level > 15";
    if (n == 0) return nullptr;
    if (entry >= n) return "entry point is not a row of the index";
    if (!levels && (max_level != 0 || n_upper_lists != 0)) return "upper levels without a level table";
    if (n_upper_lists && !adjU) return "upper lists missing";
    if (levels && levels[entry] < max_level) return "the entry point does not reach max_level";
    for (size_t v = 0; v < n; v++) {
        const uint32_t lv = levels ? levels[v] : 0;
        if (lv > 15) return "node level > 15";
        if (lv && (size_t)upper_off[v] + lv > n_upper_lists) return "upper_off + level runs past the upper lists";
        const uint32_t *l0 = adj0 + v * (size_t)M0;
        for (uint32_t j = 0; j < M0; j++)
            if (l0[j] != LEANN_EMPTY && l0[j] >= n) return "level-0 neighbour id >= n";
        for (uint32_t l = 1; l <= lv; l++) {
            const uint32_t *lu = adjU + ((size_t)upper_off[v] + l - 1) * M;
            for (uint32_t j = 0; j < M; j++) {
                const uint32_t e = lu[j];
                if (e == LEANN_EMPTY) continue;
                if (e >= n) return "upper-level neighbour id >= n";
                if (levels[e] < l) return "upper-level neighbour does not exist on that level";
            }
        }
    }
    return nullptr;
}

int leann_internal_from_host(int backend, size_t n, size_t dims, uint32_t M, uint32_t M0, uint32_t max_level, uint32_t entry,
                             const uint8_t *levels, const uint32_t *upper_off, const uint32_t *adj0, const uint32_t *adjU,
                             size_t n_upper_lists, const float *vectors, const unsigned char *feat_rows, uint32_t feat_h, uint32_t row_bytes,
                             const float *Wf32, int device, uint64_t key_offset, leann_backend **out, int row_type, const NarrowSource *narrow) {
    const bool feat = feat_rows != nullptr;
    const NarrowRows *const t = leann_internal_narrow(row_type);
    if (row_type != LEANN_ROWS_F32 && !t) {
        leann_set_error("leann_backend_from_arrays: unknown row type %d (LEANN_ROWS_F32, LEANN_ROWS_BF16 or LEANN_ROWS_I8)", row_type);
        return LEANN_ERR_INVALID;
    }
    // the rows come ONE way: recompute-on rows, host f32 `vectors`, or — a narrow type only — one of `narrow`'s two sources
    const NarrowSource src = narrow ? *narrow : NarrowSource{};
    const int ways = (vectors != nullptr) + (src.file_rows != nullptr) + (src.d_f32 != nullptr);
    bool bad = false;
    if (!t) bad = src.file_rows || src.exps || src.d_f32;                  // f32 and recompute-on handles take nothing from `narrow`
    else if (feat || ways > 1) bad = true;
    else if (src.d_f32 && src.d_ld < dims) bad = true;
    else if (t->fit ? (src.file_rows && !src.exps) : src.exps != nullptr) bad = true; // a file's exponents come with its rows, for a type that has any
    if (bad) {
        leann_set_error("leann_backend_from_arrays: invalid arguments");
        return LEANN_ERR_INVALID;
    }
    if (!out || dims == 0 || dims > 4096 || n >= (1ull << 31) || (n && ((!ways && !feat) || !adj0 || !upper_off)) ||
        (backend != LEANN_BACKEND_HNSW && backend != LEANN_BACKEND_DISKANN) ||
        (feat && (!Wf32 || feat_h == 0 || (feat_h & 3) || feat_h > 1024 || row_bytes < 2 * feat_h + 4 || (row_bytes & 7)))) {
        leann_set_error("leann_backend_from_arrays: invalid arguments");
        return LEANN_ERR_INVALID;
    }
    if (const char *why = validate_graph(n, M, M0, max_level, entry, levels, upper_off, adj0, adjU, n_upper_lists)) {
        leann_set_error("leann_backend_from_arrays: inconsistent graph arrays: %s", why);
        return LEANN_ERR_FORMAT;
    }
    if (int rc = leann_internal_check_device(device)) return rc;
    HIP_CHECK_RET(hipSetDevice(device));
    leann_backend *h = new leann_backend();
    h->kind = backend;
    h->device = device;
    h->key_offset = key_offset;
    h->g.n = n;
    h->g.d = (uint32_t)dims;
    h->g.ld = (uint32_t)((dims + 3) & ~(size_t)3);
    h->g.M = M;
    h->g.M0 = M0;
    h->g.max_level = max_level;
    h->g.entry = entry;
    if (const char *e = getenv("LEANN_VAMANA_TWO_STAGE")) h->two_stage = strcmp(e, "0") != 0; // the prune form consolidation repairs with
    // every allocation is a member of the handle or a local, so that one leann_backend_close frees whatever a failure leaves behind
    auto fail = [&](const char *what) { // (null: a failed step that has set the message)
        if (what) leann_set_error("leann_backend_from_arrays: %s failed: %s", what, hipGetErrorString(hipGetLastError()));
        leann_backend_close(h);
        return LEANN_ERR_DEVICE;
    };
    const size_t nn = std::max<size_t>(n, 1), ld = h->g.ld;
    GraphStore &st = h->store;
    if (feat) {
        h->g.feat_h = feat_h;
        DeviceBuf<unsigned char> rows;
        if (feat_h == 256) { // split device layout (GraphView::norms): 512-B rows of whole lines, norms beside them
            h->g.row_bytes = 512;
            if (rows.alloc(nn * 512) || st.norms.alloc(nn)) return fail(nullptr);
            h->g.norms = st.norms;
            const size_t slab = (size_t)1 << 20; // de-interleaved on the host, uploaded contiguously
            std::vector<unsigned char> fr(std::min(slab, nn) * 512);
            std::vector<float> nr(std::min(slab, nn));
            for (size_t s0 = 0; s0 < n; s0 += slab) {
                const size_t m = std::min(slab, n - s0);
                for (size_t i = 0; i < m; i++) {
                    memcpy(fr.data() + i * 512, feat_rows + (s0 + i) * row_bytes, 512);
                    memcpy(&nr[i], feat_rows + (s0 + i) * row_bytes + 512, 4);
                }
                if (hipMemcpy(rows + s0 * 512, fr.data(), m * 512, hipMemcpyHostToDevice) != hipSuccess ||
                    hipMemcpy(st.norms + s0, nr.data(), m * 4, hipMemcpyHostToDevice) != hipSuccess)
                    return fail("upload of the feature rows");
            }
        } else {
            h->g.row_bytes = row_bytes;
            if (rows.alloc(nn * row_bytes)) return fail(nullptr);
            if (n && hipMemcpy(rows, feat_rows, n * (size_t)row_bytes, hipMemcpyHostToDevice) != hipSuccess) return fail("upload of the feature rows");
        }
        leann_internal_own_rows(h, std::move(rows));
        if (h->Wf32.alloc((size_t)feat_h * dims)) return fail(nullptr);
        if (hipMemcpy(h->Wf32, Wf32, (size_t)feat_h * dims * 4, hipMemcpyHostToDevice) != hipSuccess) return fail("upload of the weights");
    } else if (t) {
        const int rc = leann_internal_narrow_adopt(h, t, vectors, src, src.d_f32 ? "leann_backend_to_rows" : "leann_backend_from_arrays_rows");
        if (rc) { leann_backend_close(h); return rc; }
    } else {
        DeviceBuf<float> rows;
        if (rows.alloc(std::max<size_t>(n * ld, 4))) return fail(nullptr);
        if (leann_internal_stage_rows(rows, ld, vectors, dims, dims, n, true) != hipSuccess) return fail("upload of the rows");
        leann_internal_own_rows(h, std::move(rows));
    }
    if (leann_internal_alloc_graph_lists(h, n_upper_lists)) return fail(nullptr);
    if (n) {
        if (hipMemcpy(st.adj0, adj0, n * M0 * 4, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(st.upper_off, upper_off, n * 4, hipMemcpyHostToDevice) != hipSuccess ||
            (levels ? hipMemcpy(st.levels, levels, n, hipMemcpyHostToDevice) : hipMemset(st.levels, 0, n)) != hipSuccess ||
            (n_upper_lists && hipMemcpy(st.adjU, adjU, n_upper_lists * M * 4, hipMemcpyHostToDevice) != hipSuccess))
            return fail("upload of the graph arrays");
    }
    if (hipDeviceSynchronize() != hipSuccess) return fail("hipDeviceSynchronize"); // the fills above are null-stream work; searches run on non-blocking streams
    leann_internal_sync_planes(h);
    *out = h;
    return LEANN_OK;
}
