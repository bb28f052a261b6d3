// meta.hip — metadata filters evaluated on the device from a columnar store (include/leann_backend.h "metadata filters
// evaluated on the device").  The reference's IndexSearcher answers a filter by parsing every passage's JSON and calling
// MetadataFilter::matches on it (src/index/filter.rs:319-373); here the passages' fields are columns in HBM — tag u8, number f64,
// string code u32 per row — and one kernel evaluates the compiled filter (meta_plan.h: the reduction of every op to a tag mask, a
// number test and a code test) for all rows into an allow-bitmap, which every filtered search of the library takes as it is.
//
// meta_eval_kernel: a wave takes 64 consecutive rows per step, lane = row, so a column's loads are coalesced (64 B of tags, 256 B of
// codes, 512 B of numbers per wave instruction).  A condition's outcome over the 64 rows is one __ballot; the AND / OR program folds
// those wave-uniform masks on a small stack.  Masks and stack live in LDS (328 B per wave) because the program indexes them by
// instruction: in registers that indexing would go through scratch.  Every lane writes the same value to the same LDS word and reads
// back what it wrote, so no barrier is needed.  Conditions come grouped by column: a column's tag is read once per step, its number /
// code only by the lanes whose tag says NUMBER / STRING and only if some condition tests them.  The answer is ANDed with the row's
// validity and an optional second bitmap, written as 8 single bytes per step (a caller's bitmap need not be aligned, and no byte
// behind ceil(n / 8) is written: rows behind n are never allowed, so pad bits are zero), and counted: popcount per step, one atomic per
// workgroup.  Small: 1 + 8 or 4 bytes per row and column touched, 1/8 byte out.  Measured (profiles/meta_filter.md) it is bound by the
// latency of a step's dependent loads — tag, then number or code — not by bandwidth: 0.09 ms for one column of 10M rows.
#include "common.cuh"
#include "../../include/leann_backend.h"
#include "internal.h"
#include "meta_plan.h"
#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#define META_WAVES 4      // per workgroup
#define META_MAX_GRID 2048

struct MetaColumn {
    std::string field;
    std::vector<std::string> dict; // distinct strings, bytewise ascending: read by the filter compiler only
    DeviceBuf<uint8_t> tag;
    DeviceBuf<double> num;    // empty when no row is a NUMBER
    DeviceBuf<uint32_t> code; // empty when no row is a STRING
};
struct leann_meta {
    int device = 0;
    size_t n = 0;
    DeviceBuf<uint8_t> valid; // empty: every row is valid
    mutable std::mutex mu;    // columns, words
    std::vector<std::unique_ptr<MetaColumn>> cols;
    mutable std::map<hipStream_t, DeviceBuf<uint32_t>> words; // per stream: the number sets and bitsets of the evaluation enqueued last
};

struct MetaKernelArgs {
    MetaProgram P;
    const uint8_t *tag[MP_MAX_COLS];
    const double *num[MP_MAX_COLS];
    const uint32_t *code[MP_MAX_COLS];
    const uint32_t *words;
    const uint8_t *valid, *extra; // optional bitmaps ANDed in, in this order
    uint8_t *out;
    uint32_t *count; // optional, zero at launch
    uint64_t n;
};

__global__ void __launch_bounds__(64 * META_WAVES) meta_eval_kernel(const MetaKernelArgs a) {
    __shared__ unsigned long long cmask[META_WAVES][MP_MAX_CONDS];
    __shared__ unsigned long long stack[META_WAVES][MP_MAX_DEPTH + 1];
    __shared__ uint32_t wave_count[META_WAVES];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t n_steps = (a.n + 63) / 64, n_bytes = (a.n + 7) / 8;
    uint32_t allowed = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * META_WAVES + w; g < n_steps; g += (uint64_t)gridDim.x * META_WAVES) {
        const uint64_t row = g * 64 + lane;
        bool ok = row < a.n;
        if (ok && a.valid) ok = (a.valid[row >> 3] >> (row & 7)) & 1;
        if (ok && a.extra) ok = (a.extra[row >> 3] >> (row & 7)) & 1;
        unsigned long long res = __ballot(ok);
        if (res) { // (wave-uniform)
            for (uint32_t s = 0; s < a.P.n_cols; s++) {
                const uint32_t tag = ok ? a.tag[s][row] : (uint32_t)LEANN_META_MISSING;
                double num = 0.0;
                uint32_t code = 0;
                if (tag == LEANN_META_NUMBER && (a.P.col_need[s] & 1)) num = a.num[s][row];
                if (tag == LEANN_META_STRING && (a.P.col_need[s] & 2)) code = a.code[s][row];
                for (uint32_t i = a.P.col_first[s]; i < a.P.col_first[s + 1]; i++)
                    cmask[w][i] = __ballot(meta_cond_test(a.P.cond[i], a.words, tag, num, code));
            }
            res &= meta_run_program<unsigned long long>(a.P, stack[w], [&](uint32_t i) { return cmask[w][i]; });
        }
        const uint64_t byte = g * 8 + lane;
        if (lane < 8 && byte < n_bytes) a.out[byte] = (uint8_t)(res >> (8 * lane));
        allowed += (uint32_t)__popcll(res);
    }
    if (lane == 0) wave_count[w] = allowed;
    __syncthreads();
    if (threadIdx.x == 0 && a.count) {
        uint32_t sum = 0;
        for (int i = 0; i < META_WAVES; i++) sum += wave_count[i];
        if (sum) atomicAdd(a.count, sum);
    }
}

// ---- the store -----------------------------------------------------------------------------------------------------------------
extern "C" int leann_meta_create(size_t n, const uint8_t *valid, int device, leann_meta **out) {
    if (!out) { leann_set_error("leann_meta_create: null out"); return LEANN_ERR_INVALID; }
    *out = nullptr;
    if (n >= (1ull << 32)) { leann_set_error("leann_meta_create: n = %zu is 2^32 or more", n); return LEANN_ERR_INVALID; }
    if (int rc = leann_internal_check_device(device)) return rc;
    HIP_CHECK_RET(hipSetDevice(device));
    std::unique_ptr<leann_meta> m(new leann_meta());
    m->device = device;
    m->n = n;
    if (valid && n) {
        if (int rc = m->valid.alloc((n + 7) / 8)) return rc;
        HIP_CHECK_RET(hipMemcpy(m->valid, valid, (n + 7) / 8, hipMemcpyHostToDevice));
    }
    *out = m.release();
    return LEANN_OK;
}

extern "C" int leann_meta_add_column(leann_meta *m, const char *field, const uint8_t *tag, const double *num, const char *str_blob,
                                     const uint64_t *str_off) {
    if (!m || !field || (m->n && !tag)) { leann_set_error("leann_meta_add_column: null store, field or tag"); return LEANN_ERR_INVALID; }
    const size_t n = m->n;
    size_t n_num = 0, n_str = 0;
    for (size_t i = 0; i < n; i++) {
        if (tag[i] > LEANN_META_OTHER) {
            leann_set_error("leann_meta_add_column: tag[%zu] = %u is above LEANN_META_OTHER", i, (unsigned)tag[i]);
            return LEANN_ERR_INVALID;
        }
        n_num += tag[i] == LEANN_META_NUMBER;
        n_str += tag[i] == LEANN_META_STRING;
    }
    if (n_num && !num) { leann_set_error("leann_meta_add_column: %zu NUMBER rows but num is null", n_num); return LEANN_ERR_INVALID; }
    if (n_str && !str_off) { leann_set_error("leann_meta_add_column: %zu STRING rows but str_off is null", n_str); return LEANN_ERR_INVALID; }
    if (str_off) {
        for (size_t i = 0; i < n; i++)
            if (str_off[i + 1] < str_off[i]) {
                leann_set_error("leann_meta_add_column: str_off is not monotone at row %zu", i);
                return LEANN_ERR_INVALID;
            }
        if (n && str_off[n] > str_off[0] && !str_blob) { leann_set_error("leann_meta_add_column: str_off names bytes but str_blob is null"); return LEANN_ERR_INVALID; }
    }
    std::lock_guard<std::mutex> lk(m->mu);
    for (const auto &c : m->cols)
        if (c->field == field) { leann_set_error("leann_meta_add_column: duplicate field '%s'", field); return LEANN_ERR_INVALID; }
    if (m->cols.size() >= 65535) { leann_set_error("leann_meta_add_column: the store already holds 65535 columns"); return LEANN_ERR_INVALID; }
    try {
        std::unique_ptr<MetaColumn> col(new MetaColumn());
        col->field = field;
        // dictionary: the STRING rows ordered by their bytes (memcmp, a proper prefix first), then one sweep that numbers the distinct ones
        std::vector<uint32_t> codes;
        if (n_str) {
            std::vector<uint32_t> idx;
            idx.reserve(n_str);
            for (size_t i = 0; i < n; i++)
                if (tag[i] == LEANN_META_STRING) idx.push_back((uint32_t)i);
            auto cmp = [&](uint32_t x, uint32_t y) {
                const size_t lx = str_off[x + 1] - str_off[x], ly = str_off[y + 1] - str_off[y];
                const int c = memcmp(str_blob + str_off[x], str_blob + str_off[y], std::min(lx, ly));
                return c ? c : (lx < ly ? -1 : (lx > ly ? 1 : 0));
            };
            std::sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return cmp(x, y) < 0; });
            codes.assign(n, 0);
            for (size_t j = 0; j < idx.size(); j++) {
                if (j == 0 || cmp(idx[j - 1], idx[j]) != 0)
                    col->dict.emplace_back(str_blob + str_off[idx[j]], (size_t)(str_off[idx[j] + 1] - str_off[idx[j]]));
                codes[idx[j]] = (uint32_t)(col->dict.size() - 1);
            }
        }
        HIP_CHECK_RET(hipSetDevice(m->device));
        if (int rc = col->tag.alloc(n)) return rc;
        if (n) HIP_CHECK_RET(hipMemcpy(col->tag, tag, n, hipMemcpyHostToDevice));
        if (n_num) {
            if (int rc = col->num.alloc(n)) return rc;
            HIP_CHECK_RET(hipMemcpy(col->num, num, n * 8, hipMemcpyHostToDevice));
        }
        if (n_str) {
            if (int rc = col->code.alloc(n)) return rc;
            HIP_CHECK_RET(hipMemcpy(col->code, codes.data(), n * 4, hipMemcpyHostToDevice));
        }
        m->cols.push_back(std::move(col));
    } catch (const std::bad_alloc &) {
        leann_set_error("leann_meta_add_column: out of host memory building the dictionary");
        return LEANN_ERR_INVALID;
    }
    return LEANN_OK;
}

extern "C" int leann_meta_device_enabled(void) { return leann_knobs().meta_device ? 1 : 0; }
extern "C" size_t leann_meta_len(const leann_meta *m) { return m ? m->n : 0; }
extern "C" int leann_meta_has_column(const leann_meta *m, const char *field) {
    if (!m || !field) return 0;
    std::lock_guard<std::mutex> lk(m->mu);
    for (const auto &c : m->cols)
        if (c->field == field) return 1;
    return 0;
}
extern "C" void leann_meta_close(leann_meta *m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    (void)hipDeviceSynchronize(); // an evaluation on any stream may still be reading the columns
    delete m;
}

// ---- evaluation ----------------------------------------------------------------------------------------------------------------
// compile, then enqueue on `st` (m's device is current): d_count zeroed, sets / bitsets copied into the stream's block, the kernel
static int meta_enqueue(const leann_meta *m, const leann_meta_node *nodes, size_t n_nodes, const uint8_t *d_extra, uint8_t *d_out,
                        uint32_t *d_count, hipStream_t st) {
    MetaKernelArgs a{};
    std::vector<uint32_t> words;
    {
        std::lock_guard<std::mutex> lk(m->mu);
        std::vector<MetaColumnRef> refs;
        refs.reserve(m->cols.size());
        for (const auto &c : m->cols) refs.push_back(MetaColumnRef{c->field, &c->dict});
        std::string err;
        if (int rc = meta_compile(nodes, n_nodes, refs, &a.P, &words, &err)) {
            leann_set_error("%s", err.c_str());
            return rc;
        }
        for (uint32_t s = 0; s < a.P.n_cols; s++) {
            const MetaColumn &c = *m->cols[a.P.col_id[s]];
            a.tag[s] = c.tag;
            a.num[s] = c.num;   // null: no NUMBER row, never read
            a.code[s] = c.code; // null: no STRING row, never read
        }
        if (!words.empty()) {
            DeviceBuf<uint32_t> &blk = m->words[st]; // grows to the stream's largest filter; growing waits for the device
            if (int rc = blk.grow(words.size())) return rc;
            a.words = blk;
        }
    }
    // (pageable host memory: the call returns once `words` has been staged, and the copy is ordered on the stream behind the
    // previous evaluation's kernel, which read the same block — a copy of this kind cannot be captured into a graph)
    if (!words.empty()) HIP_CHECK_RET(hipMemcpyAsync(const_cast<uint32_t *>(a.words), words.data(), words.size() * 4, hipMemcpyHostToDevice, st));
    if (d_count) HIP_CHECK_RET(hipMemsetAsync(d_count, 0, 4, st));
    a.valid = m->valid;
    a.extra = d_extra;
    a.out = d_out;
    a.count = d_count;
    a.n = m->n;
    const uint64_t n_steps = (m->n + 63) / 64;
    const unsigned grid = (unsigned)std::min<uint64_t>(std::max<uint64_t>((n_steps + META_WAVES - 1) / META_WAVES, 1), META_MAX_GRID);
    hipLaunchKernelGGL(meta_eval_kernel, dim3(grid), dim3(64 * META_WAVES), 0, st, a);
    HIP_CHECK_RET(hipGetLastError());
    return LEANN_OK;
}

extern "C" int leann_meta_eval_device(const leann_meta *m, const leann_meta_node *nodes, size_t n_nodes, const uint8_t *d_and,
                                      uint8_t *d_bitmap, uint32_t *d_n_allowed, void *stream) {
    if (!m || !nodes || !d_bitmap) { leann_set_error("leann_meta_eval_device: null store, nodes or d_bitmap"); return LEANN_ERR_INVALID; }
    HIP_CHECK_RET(hipSetDevice(m->device));
    return meta_enqueue(m, nodes, n_nodes, d_and, d_bitmap, d_n_allowed, (hipStream_t)stream);
}

extern "C" int leann_meta_eval(const leann_meta *m, const leann_meta_node *nodes, size_t n_nodes, uint8_t *bitmap, size_t *n_allowed) {
    if (n_allowed) *n_allowed = 0;
    if (!m || !nodes || (m->n && !bitmap)) { leann_set_error("leann_meta_eval: null store, nodes or bitmap"); return LEANN_ERR_INVALID; }
    HIP_CHECK_RET(hipSetDevice(m->device));
    const size_t nbytes = (m->n + 7) / 8;
    DeviceBuf<uint8_t> d_out;
    DeviceBuf<uint32_t> d_count;
    if (int rc = d_out.alloc(nbytes)) return rc;
    if (int rc = d_count.alloc(1)) return rc;
    if (int rc = meta_enqueue(m, nodes, n_nodes, nullptr, d_out, d_count, nullptr)) return rc;
    uint32_t count = 0;
    if (nbytes) HIP_CHECK_RET(hipMemcpy(bitmap, d_out, nbytes, hipMemcpyDeviceToHost));
    HIP_CHECK_RET(hipMemcpy(&count, d_count, 4, hipMemcpyDeviceToHost));
    if (n_allowed) *n_allowed = count;
    return LEANN_OK;
}

extern "C" int leann_backend_filter_create_meta(const leann_backend *hc, const leann_meta *m, const leann_meta_node *nodes, size_t n_nodes,
                                                leann_filter **out) {
    if (!hc || !m || !nodes || !out) { leann_set_error("leann_backend_filter_create_meta: null argument"); return LEANN_ERR_INVALID; }
    *out = nullptr;
    if (m->n != hc->g.n) {
        leann_set_error("leann_backend_filter_create_meta: the store holds %zu rows, the index %zu", m->n, (size_t)hc->g.n);
        return LEANN_ERR_INVALID;
    }
    if (m->device != hc->device) {
        leann_set_error("leann_backend_filter_create_meta: the store is on device %d, the index on device %d", m->device, hc->device);
        return LEANN_ERR_INVALID;
    }
    if (hc->sharded) { // evaluated once on the store's device, then the per-shard registration of leann_backend_filter_create
        std::vector<uint8_t> bitmap(std::max<size_t>((m->n + 7) / 8, 1));
        if (int rc = leann_meta_eval(m, nodes, n_nodes, bitmap.data(), nullptr)) return rc;
        return leann_backend_filter_create(hc, bitmap.data(), out);
    }
    leann_filter *f = nullptr;
    if (int rc = leann_internal_filter_begin(hc, "leann_backend_filter_create_meta", &f)) return rc;
    int rc = meta_enqueue(m, nodes, n_nodes, nullptr, f->d_allow, nullptr, nullptr);
    if (rc == LEANN_OK && hipStreamSynchronize(nullptr) != hipSuccess) {
        leann_set_error("leann_backend_filter_create_meta: the evaluation failed on the device");
        rc = LEANN_ERR_DEVICE;
    }
    if (rc != LEANN_OK) { delete f; return rc; }
    return leann_internal_filter_finish(hc, f, out);
}
