// api.hip — C ABI (include/leann_backend.h) over the gfx950 kernels: errors, logging and knobs, raw device helpers, closing a
// handle, the search entry points with their host<->HBM staging, kernel dispatch, request coalescing, registered filters, graph export.
// (Making a handle: handle.hip; index files: indexfile.hip.)  No CPU fallback exists in this library by design: every
// search / scan / build entry point runs HIP kernels or returns LEANN_ERR_DEVICE.
#include "common.cuh"
#include "search.cuh"
#include "../../include/leann_backend.h"
#include "internal.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <strings.h>
#include <map>
#include <mutex>
#include <string>
#include <vector>
#include <sys/stat.h>
#include <chrono>
#include <condition_variable>
#include <thread>

static thread_local char g_err[2048] = "";
extern "C" void leann_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char *leann_last_error(void) { return g_err; }
bool leann_log_enabled(int level) {
    static const int threshold = [] {
        const char *e = getenv("LEANN_LOG");
        if (!e) return (int)LEANN_LOG_WARN;
        if (!strcasecmp(e, "error")) return (int)LEANN_LOG_ERROR;
        if (!strcasecmp(e, "info")) return (int)LEANN_LOG_INFO;
        if (!strcasecmp(e, "debug") || !strcasecmp(e, "trace")) return (int)LEANN_LOG_DEBUG;
        return (int)LEANN_LOG_WARN;
    }();
    return level <= threshold;
}
void leann_log(int level, const char *fmt, ...) {
    if (!leann_log_enabled(level)) return;
    static const char *names[] = {"ERROR", "WARN", "INFO", "DEBUG"};
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    fprintf(stderr, "%s leann_hip: %s\n", names[level < 0 ? 0 : (level > 3 ? 3 : level)], buf);
}
extern "C" const char *leann_version(void) { return "leann-rs_amd 0.1 (gfx950)"; }

// ---- environment knobs: read once (internal.h) -----------------------------------------------------
static LeannKnobs *read_knobs_from_env() {
    LeannKnobs *k = new LeannKnobs();
    auto num = [](const char *name, int lo, int hi) { const char *e = getenv(name); if (!e || !*e) return 0; int v = atoi(e); return v >= lo && v <= hi ? v : 0; };
    auto flag = [](const char *name) { const char *e = getenv(name); return e && *e && strcmp(e, "0") != 0; };
    k->hash_bits = num("LEANN_DEBUG_HASH_BITS", 6, 15);
    k->nw = num("LEANN_DEBUG_NW", 1, 64);
    k->gpool_bits = num("LEANN_DEBUG_GPOOL_BITS", 6, 31);
    k->gpool2_bits = num("LEANN_DEBUG_GPOOL2_BITS", 6, 31);
    k->no_feat256 = flag("LEANN_DEBUG_NO_FEAT256");
    k->no_zero_copy = flag("LEANN_DEBUG_NO_ZERO_COPY");
    k->no_emit = flag("LEANN_DEBUG_NO_EMIT");
    k->fused_v1 = flag("LEANN_DEBUG_FUSED_V1");
    k->no_list = flag("LEANN_RECOMPUTE_NO_LIST");
    k->no_tiled = flag("LEANN_RECOMPUTE_NO_TILED");
    k->hnsw_reference_ef = flag("LEANN_HNSW_REFERENCE_EF");
    k->force_remote = flag("LEANN_DEBUG_FORCE_REMOTE");
    if (const char *e = getenv("LEANN_ROW_SCREEN")) k->row_screen = (!strcmp(e, "0") || !strcasecmp(e, "off")) ? 0 : (!strcmp(e, "1") || !strcasecmp(e, "on")) ? 2 : 1;
    if (const char *e = getenv("LEANN_COALESCE")) k->coalesce_off = !strcmp(e, "off") || !strcmp(e, "0");
    if (const char *e = getenv("LEANN_STAMP_BUF")) k->stamp_buf = strtoull(e, nullptr, 0);
    if (const char *e = getenv("LEANN_META_DEVICE")) k->meta_device = strcmp(e, "0") != 0;
    if (const char *e = getenv("LEANN_DEBUG_META_BATCH_BYTES")) k->meta_batch_bytes = strtoull(e, nullptr, 0);
    return k;
}
static std::atomic<const LeannKnobs *> g_knobs{nullptr};
const LeannKnobs &leann_knobs() {
    const LeannKnobs *k = g_knobs.load(std::memory_order_acquire);
    if (!k) {
        LeannKnobs *fresh = read_knobs_from_env();
        const LeannKnobs *expected = nullptr;
        if (g_knobs.compare_exchange_strong(expected, fresh, std::memory_order_acq_rel)) k = fresh;
        else { delete fresh; k = expected; }
    }
    return *k;
}
// test hook: re-read the environment (the previous struct is left alive on purpose: a search in flight may still be reading it)
extern "C" void leann_debug_reload_env(void) { g_knobs.store(read_knobs_from_env(), std::memory_order_release); }
// test hook: device blocks the library owns now, through a DeviceBuf or a ScratchLease (blocks idle in the scratch pool do not count)
std::atomic<uint64_t> leann_internal_device_blocks{0};
extern "C" uint64_t leann_debug_device_blocks(void) { return leann_internal_device_blocks.load(); }

// ---- raw device helpers ---------------------------------------------------------------------------
extern "C" int leann_device_count(int *n) {
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { c = 0; (void)hipGetLastError(); }
    *n = c;
    return LEANN_OK;
}
extern "C" int leann_device_malloc(int device, size_t bytes, void **out) {
    HIP_CHECK_RET(hipSetDevice(device));
    HIP_CHECK_RET(hipMalloc(out, bytes ? bytes : 16));
    return LEANN_OK;
}
extern "C" int leann_device_free(void *p) {
    if (p) HIP_CHECK_RET(hipFree(p));
    return LEANN_OK;
}
// the two functions every DeviceBuf (device_mem.h) allocates and frees through
void *leann_internal_device_alloc(size_t bytes) {
    void *p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    leann_internal_device_blocks++;
    return p;
}
void leann_internal_device_release(void *p) {
    if (p) leann_internal_device_blocks--;
    (void)hipFree(p);
}
int leann_internal_check_device(int device) {
    int ndev = 0;
    leann_device_count(&ndev);
    if (device >= 0 && device < ndev) return LEANN_OK;
    leann_set_error("HIP device %d not available (%d visible). This library has no CPU fallback.", device, ndev);
    return LEANN_ERR_DEVICE;
}
extern "C" int leann_device_upload(void *d, const void *h, size_t bytes) {
    HIP_CHECK_RET(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice));
    return LEANN_OK;
}
extern "C" int leann_device_download(void *h, const void *d, size_t bytes) {
    HIP_CHECK_RET(hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost));
    return LEANN_OK;
}
extern "C" int leann_device_sync(int device) {
    HIP_CHECK_RET(hipSetDevice(device));
    HIP_CHECK_RET(hipDeviceSynchronize());
    return LEANN_OK;
}

extern "C" int leann_backend_set_coalescing(leann_backend *h, uint32_t wait_us, uint32_t max_batch);
// ---- handle (structs in internal.h) ---------------------------------------------------------------
Workspace::~Workspace() { // (the six buffers free themselves)
    if (pin) (void)hipHostFree(pin);
    if (stream) (void)hipStreamDestroy(stream);
}
static uint32_t debug_bits(int knob, uint32_t lo, uint32_t hi, uint32_t dflt) { // test hooks: force tiny visited tables
    return knob >= (int)lo && knob <= (int)hi ? (uint32_t)knob : dflt;
}
// Pool 1: GPOOL_TABLES tables of 2^GPOOL_BITS slots (512 MB) for queries that outgrow their LDS table.  Pool 2, only when the
// index has more rows than a pool-1 table holds at 75 % load: a few tables of >= (n + 128) / 0.75 slots each (<= 1 GiB in all), so
// that no search can run out of visited-set space whatever the beam (search.cuh).
static int ensure_gpool(leann_backend *h) {
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->gpool) return LEANN_OK;
    DeviceBuf<unsigned long long> p, p2; // this call's own until the last lines: a failing return frees them
    DeviceBuf<uint32_t> lock, lock2;
    const uint32_t bits = debug_bits(leann_knobs().gpool_bits, 6, GPOOL_BITS, GPOOL_BITS), tables = GPOOL_TABLES;
    const size_t slots = (size_t)tables << bits;
    uint32_t bits2 = 0, tables2 = 0;
    const uint64_t need = h->g.n + 128;
    if (need > (1ull << bits) - (1ull << (bits - 2))) {
        bits2 = bits + 1;
        while (bits2 < 31 && (1ull << bits2) - (1ull << (bits2 - 2)) < need) bits2++;
        bits2 = debug_bits(leann_knobs().gpool2_bits, 6, 31, bits2);
        const uint64_t per = 8ull << bits2;
        tables2 = (uint32_t)std::min<uint64_t>(64, std::max<uint64_t>(2, (1ull << 30) / per));
    }
    auto fail = [&](const char *what) {
        leann_set_error("visited-table pool: %s failed: %s", what, hipGetErrorString(hipGetLastError()));
        return LEANN_ERR_DEVICE;
    };
    if (p.alloc(slots) || lock.alloc(tables + 4)) return LEANN_ERR_DEVICE;
    if (hipMemset(p, 0, slots * 8) != hipSuccess) return fail("hipMemset"); // generation 0 is never issued
    if (hipMemset(lock, 0, (tables + 4) * 4) != hipSuccess) return fail("hipMemset");
    if (tables2) {
        if (p2.alloc((size_t)tables2 << bits2) || lock2.alloc(tables2)) return LEANN_ERR_DEVICE;
        if (hipMemset(p2, 0, ((size_t)tables2 << bits2) * 8) != hipSuccess) return fail("hipMemset");
        if (hipMemset(lock2, 0, tables2 * 4) != hipSuccess) return fail("hipMemset");
    }
    // hipMemset on device memory returns before the fill has run (it is queued on the null stream), and searches run on NON-BLOCKING
    // streams, which do not wait for the null stream: without this wait the first launch could migrate queries into a table that was
    // still being zeroed under them (entries lost -> nodes visited twice -> results off the oracle's; seen once the migration came a
    // few microseconds earlier, tests/test_gpu_parity.py::test_visited_table_overflow_moves_to_hbm_pool).  Once per handle.
    if (hipDeviceSynchronize() != hipSuccess) return fail("hipDeviceSynchronize");
    h->gpool_lock = std::move(lock); // now belong to the handle
    h->gpool_ctr = h->gpool_lock + tables;
    h->gpool_bits = bits;
    h->gpool_tables = tables;
    h->gpool2 = std::move(p2);
    h->gpool2_lock = std::move(lock2);
    h->gpool2_bits = bits2;
    h->gpool2_tables = tables2;
    h->gpool = std::move(p);
    return LEANN_OK;
}
static void set_pool_args(const leann_backend *h, SearchArgs &a) {
    a.gpool = h->gpool; a.gpool_lock = h->gpool_lock; a.gpool_ctr = h->gpool_ctr;
    a.gpool_bits = h->gpool_bits; a.gpool_tables = h->gpool_tables;
    a.gpool2 = h->gpool2; a.gpool2_lock = h->gpool2_lock; a.gpool2_bits = h->gpool2_bits; a.gpool2_tables = h->gpool2_tables;
}

extern "C" void leann_backend_close(leann_backend *h) {
    if (!h) return;
    leann_backend_set_coalescing(h, 0, 0); // stops the dispatcher thread, if any
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize(); // before anything the handle owns is freed, here or in `delete h`: no stream still runs on it
    h->free_ws.clear();
    if (h->sharded) leann_sharded_close(h->sharded); // composite handle: the sub-indexes own the device memory
    else leann_internal_free_planes(h);              // (for its log line)
    delete h; // every device block of the handle is a member that frees itself
}
extern "C" size_t leann_backend_len(const leann_backend *h) { return h ? (size_t)h->g.n : 0; }
extern "C" size_t leann_backend_dims(const leann_backend *h) { return h ? (size_t)h->g.d : 0; }
extern "C" const float *leann_backend_device_rows(const leann_backend *h) { return h && !h->sharded && !leann_internal_narrow_rows(h) ? h->g.X : nullptr; }
#define NOT_ON_SHARDED(h, what)                                                                                                    \
    do {                                                                                                                           \
        if ((h) && (h)->sharded) {                                                                                                 \
            leann_set_error("%s is not available on a sharded handle (use leann_backend_shard(h, g) for one shard's)", what);       \
            return LEANN_ERR_UNSUPPORTED;                                                                                          \
        }                                                                                                                          \
    } while (0)

extern "C" int leann_backend_stats(const leann_backend *hc, leann_search_stats *out, int reset) {
    leann_backend *h = const_cast<leann_backend *>(hc);
    if (!h || !out) { leann_set_error("leann_backend_stats: null argument"); return LEANN_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(h->mu);
    *out = h->stats;
    if (reset) h->stats = leann_search_stats{};
    return LEANN_OK;
}

// Reference-exact mode: the reference's HNSW searcher is opened with expansion_search = 64
// (src/backend/hnsw.rs:49) and drops the caller's `complexity` (`_complexity`, :83), so every `leann search --complexity N` runs at
// ef = max(64, top_k).  LEANN_HNSW_REFERENCE_EF=1 in the environment when the handle is made latches that behaviour into it (HNSW
// handles only; DiskANN honours complexity in the reference too, diskann.rs:54).  Default: complexity is honoured.
size_t leann_internal_effective_complexity(const leann_backend *h, size_t complexity) {
    return (h->fixed_ef && h->kind == LEANN_BACKEND_HNSW) ? (size_t)h->fixed_ef : complexity;
}

// ---- kernel dispatch --------------------------------------------------------------------------------
// Which kernel a call runs is decided by search_plan (search_plan.h); the table below holds every traversal kernel this file compiles
// — F32, SCREEN, FEAT and FEAT256; the bf16 rows' kernels have a table of their own (search_bf16.hip) —, one row per kernel, the key
// and the instantiation written from the same template arguments.
template <int FAMILY, int T, int R, int NW, bool WIDE, bool FILT, bool BUILD>
static constexpr SearchKernelRow search_row() {
    SearchKernel k = nullptr;
    if constexpr (FAMILY == SEARCH_SCREEN) k = beam_search_screen_kernel<T, R>;
    else if constexpr (FAMILY == SEARCH_F32 && WIDE) k = FILT ? wide_beam_search_filtered_kernel<T, R, NW> : wide_beam_search_kernel<T, R, NW, BUILD>;
    else if constexpr (FAMILY == SEARCH_F32) k = FILT ? beam_search_filtered_kernel<T, R, NW> : beam_search_kernel<T, R, NW, BUILD>;
    else if constexpr (FAMILY == SEARCH_FEAT && WIDE) k = FILT ? wide_beam_search_feat_filtered_kernel<T, R, NW> : wide_beam_search_feat_kernel<T, R, NW>;
    else if constexpr (FAMILY == SEARCH_FEAT) k = FILT ? beam_search_feat_filtered_kernel<T, R, NW> : beam_search_feat_kernel<T, R, NW>;
    else if constexpr (FAMILY == SEARCH_FEAT256 && WIDE) k = FILT ? wide_beam_search_feat256_filtered_kernel<R, NW> : wide_beam_search_feat256_kernel<R, NW>;
    else if constexpr (FAMILY == SEARCH_FEAT256) k = FILT ? beam_search_feat256_filtered_kernel<R, NW> : beam_search_feat256_kernel<R, NW>;
    return {FAMILY, T, R, NW, WIDE, FILT, BUILD, k};
}
// stored f32 rows: plain, construction and filtered form of one <T, R, NW>; 16, 8 and 4 waves, wide lists 16 and 4 only
#define F32_ROW(T, NW, WIDE, FILT, BUILD) search_row<SEARCH_F32, T, search_f32_R(T), NW, WIDE, FILT, BUILD>()
#define F32_FORMS(T, NW, WIDE) F32_ROW(T, NW, WIDE, false, false), F32_ROW(T, NW, WIDE, false, true), F32_ROW(T, NW, WIDE, true, false)
#define F32_WIDTH(T) F32_FORMS(T, 16, false), F32_FORMS(T, 8, false), F32_FORMS(T, 4, false), F32_FORMS(T, 16, true), F32_FORMS(T, 4, true)
// recompute-on rows: plain and filtered, narrow and wide lists, of one <T, R, NW> (FEAT256: <G = R, NW>, T = 1)
#define FEAT_FORMS(FAMILY, T, R, NW)                                                                                               \
    search_row<FAMILY, T, R, NW, false, false, false>(), search_row<FAMILY, T, R, NW, false, true, false>(),                       \
        search_row<FAMILY, T, R, NW, true, false, false>(), search_row<FAMILY, T, R, NW, true, true, false>()
#define FEAT_WIDTH(T) FEAT_FORMS(SEARCH_FEAT, T, search_feat_R(T), 16), FEAT_FORMS(SEARCH_FEAT, T, search_feat_R(T), 4)
static int search_kernel(const SearchPlan &p, SearchKernel *out) {
    static constexpr SearchKernelRow rows[] = {
        F32_WIDTH(1), F32_WIDTH(2), F32_WIDTH(3), F32_WIDTH(4), F32_WIDTH(6), F32_WIDTH(8), F32_WIDTH(12), F32_WIDTH(16),
        search_row<SEARCH_SCREEN, 3, LEANN_SCREEN_R3, 4, false, false, false>(), search_row<SEARCH_SCREEN, 6, LEANN_SCREEN_R6, 4, false, false, false>(),
        FEAT_WIDTH(1), FEAT_WIDTH(2), FEAT_WIDTH(4),
        FEAT_FORMS(SEARCH_FEAT256, 1, 1, 16), FEAT_FORMS(SEARCH_FEAT256, 1, LEANN_FEAT_G, 4),
    };
    return leann_internal_find_kernel(rows, p, out);
}
int launch_plan(SearchKernel kernel, const SearchPlan &p, const GraphView &g, const SearchArgs &a, hipStream_t st) {
    if (p.lds_bytes > 64 * 1024)
        HIP_CHECK_RET(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL(kernel, dim3(a.nq), dim3(p.NW * 64), p.lds_bytes, st, g, a);
    HIP_CHECK_RET(hipGetLastError());
    return LEANN_OK;
}

// recompute-on mode: queries [nq x dims] -> g = W q [nq x feat_h] into the stream's scratch (f32 MFMA, k-ordered chains)
static int project_queries(leann_backend *h, const float *d_queries, size_t nq, hipStream_t st, const float **out) {
    float *G = nullptr;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        auto &sc = h->proj_scratch[st];
        if (int rc = sc.grow(nq * h->g.feat_h)) return rc;
        G = sc;
    }
    int rc = leann_internal_score(h->Wf32, h->g.feat_h, h->g.d, h->g.d, d_queries, nq, h->g.d, G, st);
    *out = G;
    return rc;
}

int leann_internal_launch_search(leann_backend *h, SearchArgs a, hipStream_t st) {
    if (a.nq == 0) return LEANN_OK;
    const GraphView &g = h->g;
    if (a.ef < a.k) a.ef = a.k; // diskann.rs:54
    SearchShape shape{};
    shape.ld = g.ld; shape.d = g.d; shape.feat_h = g.feat_h; shape.bf16 = leann_internal_bf16(h); shape.maxdeg = std::max(g.M0, g.M);
    shape.i8 = leann_internal_i8(h);
    shape.screen_ready = !g.feat_h && !shape.bf16 && !shape.i8 && h->row_screen.load(std::memory_order_relaxed) != 0 && leann_internal_planes_ready(h) &&
                         leann_internal_screen_shape(g);
    const SearchCall call{a.nq, a.k, a.ef, a.allow != nullptr, a.q_rows != nullptr};
    const SearchKnobs knobs{leann_knobs().hash_bits, leann_knobs().nw, leann_knobs().no_feat256};
    const SearchPlan p = search_plan(shape, call, knobs);
    if (p.err) { leann_set_error("%s", p.msg); return p.err; }
    a.hash_bits = p.hash_bits;
    if (int rc = ensure_gpool(h)) return rc;
    set_pool_args(h, a);
    if (g.feat_h) { // the walk runs on the projected queries
        const float *G = nullptr;
        if (int rc = project_queries(h, a.queries, a.nq, st, &G)) return rc;
        a.queries = G;
        a.ldq = g.feat_h;
    }
    if (p.family == SEARCH_SCREEN) { a.x_hi = h->x_hi; a.x_lo = h->x_lo; a.ldp = h->ldp; a.screen_ctr = h->screen_ctr; }
    SearchKernel kernel = nullptr;
    if (int rc = p.family == SEARCH_BF16 ? leann_internal_bf16_kernel(g, p, &kernel)
                 : p.family == SEARCH_I8 ? leann_internal_i8_kernel(g, p, &kernel) : search_kernel(p, &kernel))
        return rc;
    if (leann_log_enabled(LEANN_LOG_DEBUG)) {
        char name[96];
        search_plan_name(p, name, sizeof name);
        leann_log(LEANN_LOG_DEBUG, "search: %s, hash_bits %u, lds_bytes %zu", name, p.hash_bits, p.lds_bytes);
    }
    return launch_plan(kernel, p, g, a, st);
}

extern "C" int leann_backend_search_batch_device(const leann_backend *hc, const float *d_queries, size_t nq,
                                                 size_t top_k, size_t complexity, uint64_t *d_keys, float *d_dists,
                                                 uint32_t *d_counts, uint32_t *d_stats, void *stream) {
    return leann_backend_search_filtered_batch_device(hc, d_queries, nq, top_k, complexity, nullptr, 0, d_keys, d_dists,
                                                      d_counts, d_stats, stream);
}

// The search on a plain handle (internal.h): what the filter means for this index, the live mask of removals (consolidate.hip), then
// the graph walk or the exact scan of the allowed rows (scan.hip).
int leann_internal_search_plain(leann_backend *h, const float *d_queries, size_t nq, size_t top_k, size_t complexity, const SearchFilter &f,
                                uint64_t *d_keys, float *d_dists, uint32_t *d_counts, uint32_t *d_stats, hipStream_t st) {
    if (int rc = leann_internal_check_allow_stride(f, h->g.n)) return rc;
    if (nq == 0) return LEANN_OK;
    if (f.exact && h->g.feat_h) {
        leann_set_error("exact filtered search needs stored vectors; this index recomputes them from features (use leann_recompute_search_batch_device with an allow mask)");
        return LEANN_ERR_UNSUPPORTED;
    }
    if (f.exact && leann_internal_narrow_rows(h)) {
        leann_set_error("exact filtered search scans f32 rows; this index stores %s rows (use the filtered walk: mode 0, or mode 2 which picks it)",
                        leann_internal_row_name(h));
        return LEANN_ERR_UNSUPPORTED;
    }
    if (h->g.n == 0) {
        HIP_CHECK_RET(hipMemsetAsync(d_counts, 0, nq * 4, st));
        return LEANN_OK;
    }
    // Removals: a registered filter holds live positions only (leann_backend_filter_create) and is never masked again.  Any other walk
    // runs under live AND the caller's bitmap — without a bitmap, under the live mask until the graph has been repaired —, and an
    // exact answer compacts live AND allow.
    const leann_filter *reg = f.registered;
    const uint8_t *allow = reg ? reg->d_allow : f.d_allow;
    size_t allow_stride = reg ? 0 : f.allow_stride;
    if (!reg)
        if (int rc = leann_internal_live_allow(h, allow, allow_stride, nq, !f.exact, st, &allow, &allow_stride)) return rc;
    if (f.exact) {
        if (!allow) { leann_set_error("exact filtered search: no filter given"); return LEANN_ERR_INVALID; }
        if (d_stats) HIP_CHECK_RET(hipMemsetAsync(d_stats, 0, nq * 16, st)); // no walk: no evaluations / hops to count
        if (reg) // the compacted list of allowed rows exists already
            return leann_internal_filtered_exact_list(h->g.X, h->g.d, h->g.ld, d_queries, nq, top_k, reg->d_list, reg->n_allowed, h->key_offset,
                                                      d_keys, d_dists, d_counts, st);
        return leann_internal_filtered_exact(h->g.X, h->g.n, h->g.d, h->g.ld, d_queries, nq, top_k, allow, allow_stride, h->key_offset, d_keys,
                                             d_dists, d_counts, st);
    }
    SearchArgs a{};
    a.queries = d_queries;
    a.ldq = h->g.d;
    a.nq = (uint32_t)nq;
    a.k = (uint32_t)top_k;
    a.ef = (uint32_t)std::max(leann_internal_effective_complexity(h, complexity), top_k);
    a.target_level = 0;
    a.key_offset = h->key_offset;
    a.out_keys = d_keys;
    a.out_dists = d_dists;
    a.out_counts = d_counts;
    a.out_stats = d_stats;
    a.allow = allow;
    a.allow_stride = allow_stride;
#ifdef LEANN_STAMPS
    if (const unsigned long long e = leann_knobs().stamp_buf) { // diagnostic build: [nq x 8] u64 device buffer address in the environment
        a.out_nexp = reinterpret_cast<uint32_t *>(e);
        a.exp_cap = 0xFEED;
    }
#endif
    return leann_internal_launch_search(h, a, st);
}
// a device-pointer entry point: the composite handle fans out, gathers and merges (shard.hip; d_stats stays [nq x 4]: summed over the shards)
static int search_device(leann_backend *h, const float *d_queries, size_t nq, size_t top_k, size_t complexity, const SearchFilter &f,
                         uint64_t *d_keys, float *d_dists, uint32_t *d_counts, uint32_t *d_stats, hipStream_t st) {
    HIP_CHECK_RET(hipSetDevice(h->device));
    if (h->sharded) return leann_internal_sharded_search(h->sharded, d_queries, nq, top_k, complexity, f, d_keys, d_dists, d_counts, d_stats, st, nullptr);
    return leann_internal_search_plain(h, d_queries, nq, top_k, complexity, f, d_keys, d_dists, d_counts, d_stats, st);
}

// Filtered traversal: the allow-bitmap is evaluated inside the kernel instead of the
// reference's fetch_k = 5*top_k over-fetch + post-filter (src/index/searcher.rs:129-133,:190-194).
extern "C" int leann_backend_search_filtered_batch_device(const leann_backend *hc, const float *d_queries, size_t nq,
                                                          size_t top_k, size_t complexity, const uint8_t *d_allow,
                                                          size_t allow_stride, uint64_t *d_keys, float *d_dists,
                                                          uint32_t *d_counts, uint32_t *d_stats, void *stream) {
    leann_backend *h = const_cast<leann_backend *>(hc);
    if (!h || !d_queries || !d_keys || !d_dists || !d_counts || top_k == 0) {
        leann_set_error("leann_backend_search_batch_device: null/zero argument");
        return LEANN_ERR_INVALID;
    }
    SearchFilter f;
    f.d_allow = d_allow; f.allow_stride = allow_stride;
    return search_device(h, d_queries, nq, top_k, complexity, f, d_keys, d_dists, d_counts, d_stats, (hipStream_t)stream);
}

// BackendSearcher::search batched over host pointers.
extern "C" int leann_backend_search_batch(const leann_backend *hc, const float *queries, size_t nq, size_t top_k,
                                          size_t complexity, uint64_t *keys, float *dists, uint32_t *counts) {
    return leann_backend_search_filtered_batch(hc, queries, nq, top_k, complexity, nullptr, 0, keys, dists, counts);
}

// ... with an optional allow-bitmap over positions (host memory; one shared bitmap when allow_stride == 0)
enum { FILTER_WALK = 0, FILTER_EXACT = 1, FILTER_AUTO = 2 };
static int search_filtered_batch_host(const leann_backend *hc, const float *queries, size_t nq, size_t top_k, size_t complexity,
                                      const uint8_t *allow, size_t allow_stride, uint64_t *keys, float *dists, uint32_t *counts, int mode,
                                      const leann_filter *flt = nullptr);

// The two ends of registering a filter on a plain handle, shared by leann_backend_filter_create (the bitmap is uploaded in between) and
// leann_backend_filter_create_meta (meta.hip: it is evaluated there).  begin: h's device current, a filter with room for the bitmap.
int leann_internal_filter_begin(const leann_backend *hc, const char *who, leann_filter **out) {
    *out = nullptr;
    if (hc->g.n >= (1ull << 32)) {
        leann_set_error("%s: the index has 2^32 rows or more", who);
        return LEANN_ERR_INVALID;
    }
    HIP_CHECK_RET(hipSetDevice(hc->device));
    leann_filter *f = new leann_filter();
    f->device = hc->device;
    f->n = hc->g.n;
    const size_t nbytes = std::max<size_t>((f->n + 7) / 8, 1);
    if (f->d_allow.alloc(nbytes)) {
        leann_set_error("%s: device allocation of %zu bytes failed", who, nbytes);
        delete f;
        return LEANN_ERR_DEVICE;
    }
    *out = f;
    return LEANN_OK;
}
// finish: f->d_allow holds the bitmap.  Epoch and owner, live mask, list of allowed positions; on failure f is deleted.
int leann_internal_filter_finish(const leann_backend *hc, leann_filter *f, leann_filter **out) {
    f->epoch = hc->removal_epoch;
    f->owner = hc->serial;
    int rc = leann_internal_and_live_inplace(hc, f->d_allow); // removed positions are never allowed: the bitmap and the list hold live ones only
    if (rc == LEANN_OK && f->n) rc = leann_internal_compact_allow(f->d_allow, f->n, &f->d_list, &f->n_allowed, nullptr);
    if (rc != LEANN_OK) {
        delete f;
        return rc;
    }
    *out = f;
    return LEANN_OK;
}

// Registered filters: a server that answers many queries under the same metadata filter uploads and compacts the bitmap once
// (the host-pointer calls above re-send N/8 bytes and re-compact them for every query: 1.25 MB at 10M rows).
extern "C" int leann_backend_filter_create(const leann_backend *hc, const uint8_t *allow, leann_filter **out) {
    if (!hc || !allow || !out) {
        leann_set_error("leann_backend_filter_create: null argument");
        return LEANN_ERR_INVALID;
    }
    *out = nullptr;
    if (hc->sharded) { // composite handle: one sub-filter per shard — its slice of the bitmap (shard boundaries are multiples of 64), on its device
        const size_t G = leann_internal_sharded_count(hc->sharded);
        leann_filter *f = new leann_filter();
        f->device = hc->device;
        f->n = hc->g.n;
        for (size_t g = 0; g < G; g++) {
            leann_backend *sh = leann_internal_sharded_shard(hc->sharded, g);
            const uint64_t lo = leann_internal_sharded_lo(hc->sharded, g);
            leann_filter *part = nullptr;
            int rc = (!sh || (lo & 7)) ? (leann_set_error("registered filter: shard %zu does not start at a multiple of 8", g), (int)LEANN_ERR_UNSUPPORTED)
                                       : leann_backend_filter_create(sh, allow + lo / 8, &part);
            if (rc) { leann_backend_filter_free(f); return rc; }
            f->parts.push_back(part);
            f->n_allowed += part->n_allowed;
        }
        (void)hipSetDevice(hc->device);
        f->epoch = hc->removal_epoch;
        f->owner = hc->serial;
        *out = f;
        return LEANN_OK;
    }
    leann_filter *f = nullptr;
    if (int rc = leann_internal_filter_begin(hc, "leann_backend_filter_create", &f)) return rc;
    if (hipMemcpy(f->d_allow, allow, (f->n + 7) / 8, hipMemcpyHostToDevice) != hipSuccess) {
        leann_set_error("leann_backend_filter_create: copy of %zu bytes to the device failed", (f->n + 7) / 8);
        delete f;
        return LEANN_ERR_DEVICE;
    }
    return leann_internal_filter_finish(hc, f, out);
}
extern "C" size_t leann_backend_filter_count(const leann_filter *f) { return f ? f->n_allowed : 0; }
// the registered bitmap (valid AND match AND live) for a caller that filters something else by it: the BM25 *_filtered calls
extern "C" int leann_backend_filter_bitmap_device(const leann_filter *f, const uint8_t **d_allow, size_t *n) {
    if (!f || !d_allow) {
        leann_set_error("leann_backend_filter_bitmap_device: null %s", !f ? "filter" : "d_allow");
        return LEANN_ERR_INVALID;
    }
    *d_allow = nullptr;
    if (n) *n = 0;
    if (!f->parts.empty()) {
        leann_set_error("leann_backend_filter_bitmap_device: the filter of a composite handle holds one bitmap slice per shard, each on "
                        "its shard's device, and no whole one; pass the caller's own bitmap over global positions instead");
        return LEANN_ERR_UNSUPPORTED;
    }
    *d_allow = f->d_allow;
    if (n) *n = f->n;
    return LEANN_OK;
}
extern "C" void leann_backend_filter_free(leann_filter *f) {
    if (!f) return;
    if (!f->parts.empty()) {
        for (auto *p : f->parts) leann_backend_filter_free(p);
        delete f;
        return;
    }
    (void)hipSetDevice(f->device);
    (void)hipDeviceSynchronize(); // searches on any stream may still be reading the bitmap / the list
    delete f; // the bitmap and the list go with it, on the filter's device and after the synchronisation above
}
extern "C" int leann_backend_search_filter_batch(const leann_backend *hc, const float *queries, size_t nq, size_t top_k, size_t complexity,
                                                 const leann_filter *filter, int mode, uint64_t *keys, float *dists, uint32_t *counts) {
    if (!filter || !hc || filter->n != hc->g.n || filter->device != hc->device || mode < FILTER_WALK || mode > FILTER_AUTO ||
        filter->parts.empty() != (hc->sharded == nullptr)) { // (a filter registered on a sharded handle holds one sub-filter per shard, and only those)
        leann_set_error("leann_backend_search_filter_batch: null / foreign filter (made for %zu rows, the index has %zu) or bad mode %d",
                        filter ? filter->n : (size_t)0, hc ? (size_t)hc->g.n : (size_t)0, mode);
        return LEANN_ERR_INVALID;
    }
    if (filter->owner != hc->serial) { // (same length, same device: a copy of the handle the filter was registered on)
        leann_set_error("leann_backend_search_filter_batch: filter belongs to another handle; register it on this one");
        return LEANN_ERR_INVALID;
    }
    bool stale = filter->epoch != hc->removal_epoch;
    if (hc->sharded)
        for (size_t g = 0; g < filter->parts.size() && g < leann_internal_sharded_count(hc->sharded); g++)
            stale = stale || filter->parts[g]->epoch != leann_internal_sharded_shard(hc->sharded, g)->removal_epoch;
    if (stale) {
        leann_set_error("leann_backend_search_filter_batch: filter predates a removal; register it again");
        return LEANN_ERR_INVALID;
    }
    return search_filtered_batch_host(hc, queries, nq, top_k, complexity, nullptr, 0, keys, dists, counts, mode, filter);
}

extern "C" int leann_backend_search_filtered_batch(const leann_backend *hc, const float *queries, size_t nq, size_t top_k,
                                                   size_t complexity, const uint8_t *allow, size_t allow_stride,
                                                   uint64_t *keys, float *dists, uint32_t *counts) {
    return search_filtered_batch_host(hc, queries, nq, top_k, complexity, allow, allow_stride, keys, dists, counts, FILTER_WALK);
}
// ... answered exactly: the allowed rows are compacted and scanned (scan.hip), no graph involved
extern "C" int leann_backend_search_filtered_exact_batch(const leann_backend *hc, const float *queries, size_t nq, size_t top_k,
                                                         const uint8_t *allow, size_t allow_stride, uint64_t *keys, float *dists,
                                                         uint32_t *counts) {
    if (!allow) {
        leann_set_error("leann_backend_search_filtered_exact_batch: null allow-bitmap");
        return LEANN_ERR_INVALID;
    }
    return search_filtered_batch_host(hc, queries, nq, top_k, 0, allow, allow_stride, keys, dists, counts, FILTER_EXACT);
}
extern "C" int leann_backend_search_filtered_exact_batch_device(const leann_backend *hc, const float *d_queries, size_t nq, size_t top_k,
                                                                const uint8_t *d_allow, size_t allow_stride, uint64_t *d_keys,
                                                                float *d_dists, uint32_t *d_counts, void *stream) {
    leann_backend *h = const_cast<leann_backend *>(hc);
    if (!h || !d_queries || !d_keys || !d_dists || !d_counts || !d_allow || top_k == 0) {
        leann_set_error("leann_backend_search_filtered_exact_batch_device: null/zero argument");
        return LEANN_ERR_INVALID;
    }
    SearchFilter f; // (a composite handle: every shard scans its own allowed rows; lists merged by (dist, key))
    f.d_allow = d_allow; f.allow_stride = allow_stride; f.exact = true;
    return search_device(h, d_queries, nq, top_k, 0, f, d_keys, d_dists, d_counts, nullptr, (hipStream_t)stream);
}
static int search_filtered_batch_host_impl(const leann_backend *hc, const float *queries, size_t nq, size_t top_k, size_t complexity,
                                      const uint8_t *allow, size_t allow_stride, uint64_t *keys, float *dists, uint32_t *counts, int mode,
                                      const leann_filter *flt) {
    leann_backend *h = const_cast<leann_backend *>(hc);
    // exact scan of the allowed rows, or the walk with the filter inside?  FILTER_AUTO (registered filters only: the count is known):
    // exact up to 5 % of the rows / 64k rows for small batches, 1.5 % for large ones, when the index stores vectors
    bool exact = mode == FILTER_EXACT;
    const leann_backend *first = hc && hc->sharded ? leann_internal_sharded_shard(hc->sharded, 0) : hc;
    const bool stored_vectors = first && !first->g.feat_h && !leann_internal_narrow_rows(first); // f32 rows an exact scan can read
    if (mode == FILTER_AUTO && flt && hc && stored_vectors && top_k <= 1024) {
        const double frac = nq <= 64 ? 0.05 : 0.015;
        exact = flt->n_allowed <= std::max<size_t>((size_t)(frac * (double)hc->g.n), nq <= 64 ? 65536 : 0);
    }
    if (!h || !queries || !keys || !dists || !counts) {
        leann_set_error("leann_backend_search_batch: null argument");
        return LEANN_ERR_INVALID;
    }
    if (nq == 0 || top_k == 0 || h->g.n == 0) { // nothing to search: answered on the host, no workspace, no device call
        for (size_t i = 0; i < nq; i++) counts[i] = 0;
        return LEANN_OK;
    }
    HIP_CHECK_RET(hipSetDevice(h->device));
    std::unique_ptr<Workspace> w;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        if (!h->free_ws.empty()) { w = std::move(h->free_ws.back()); h->free_ws.pop_back(); }
    }
    if (!w) w.reset(new Workspace());
    int rc = LEANN_OK;
    auto fail = [&](int code) { std::lock_guard<std::mutex> lk(h->mu); h->free_ws.push_back(std::move(w)); return code; };
    if (!w->stream) {
        if (hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking) != hipSuccess) {
            leann_set_error("hipStreamCreate failed");
            return fail(LEANN_ERR_DEVICE);
        }
    }
    const size_t d = h->g.d, qf = nq * d, no = nq * top_k;
    const size_t ns = 1; // (a composite handle reduces its per-shard counters to [nq x 4] itself, shard.hip)
    // Small call on a plain handle: zero-copy through the workspace's pinned block (internal.h).  Layout, 16-byte aligned pieces:
    const size_t o_keys = (qf * 4 + 15) & ~(size_t)15, o_dists = o_keys + no * 8, o_counts = (o_dists + no * 4 + 15) & ~(size_t)15,
                 o_stats = o_counts + ((nq * 4 + 15) & ~(size_t)15), pin_bytes = o_stats + nq * 16;
    bool zero_copy = !h->sharded && !exact && pin_bytes <= ((size_t)256 << 10) && !leann_knobs().no_zero_copy;
    if (zero_copy && w->cap_pin < pin_bytes) {
        if (w->pin) (void)hipHostFree(w->pin);
        w->pin = nullptr;
        w->cap_pin = 0;
        const size_t want = std::max<size_t>(pin_bytes, (size_t)64 << 10);
        if (hipHostMalloc((void **)&w->pin, want, hipHostMallocDefault) == hipSuccess) w->cap_pin = want;
        else { (void)hipGetLastError(); zero_copy = false; } // no pinned memory to be had: the staged path below
    }
    // (queries: read in place by up to 4 queries' workgroups — every wave of a query reads all of it, and mapped host memory is not
    // cached on the device; larger small calls copy them from the pinned block with one DMA)
    const bool zc_in = zero_copy && nq <= 4;
    if (zero_copy && !zc_in && w->d_q.grow(qf)) return fail(LEANN_ERR_DEVICE);
    if (!zero_copy && (w->d_q.grow(qf) || w->d_keys.grow(no) || w->d_dists.grow(no) || w->d_counts.grow(nq) || w->d_stats.grow(ns * nq * 4)))
        return fail(LEANN_ERR_DEVICE);
    hipStream_t st = w->stream;
    if (allow) {
        const size_t total = allow_stride ? allow_stride * nq : (h->g.n + 7) / 8;
        if (w->d_allow.grow(total)) return fail(LEANN_ERR_DEVICE);
        if (hipMemcpyAsync(w->d_allow, allow, total, hipMemcpyHostToDevice, st) != hipSuccess) {
            leann_set_error("H2D copy of the allow-bitmap failed");
            return fail(LEANN_ERR_DEVICE);
        }
    }
    if (zero_copy) memcpy(w->pin, queries, qf * 4);
    if (!zc_in && hipMemcpyAsync(w->d_q, zero_copy ? reinterpret_cast<const float *>(w->pin) : queries, qf * 4, hipMemcpyHostToDevice, st) != hipSuccess) {
        leann_set_error("H2D copy of queries failed");
        return fail(LEANN_ERR_DEVICE);
    }
    // one search: the same decision (exact / walk) for a plain handle and for every shard of a composite one
    SearchFilter f;
    f.exact = exact;
    if (flt) f.registered = flt;
    else if (allow) { f.d_allow = w->d_allow; f.allow_stride = allow_stride; }
    const float *d_q = zc_in ? reinterpret_cast<const float *>(w->pin) : w->d_q;
    uint64_t *d_keys = zero_copy ? reinterpret_cast<uint64_t *>(w->pin + o_keys) : w->d_keys;
    float *d_dists = zero_copy ? reinterpret_cast<float *>(w->pin + o_dists) : w->d_dists;
    uint32_t *d_counts = zero_copy ? reinterpret_cast<uint32_t *>(w->pin + o_counts) : w->d_counts;
    uint32_t *d_stats = zero_copy ? reinterpret_cast<uint32_t *>(w->pin + o_stats) : w->d_stats;
    rc = h->sharded ? leann_internal_sharded_search(h->sharded, d_q, nq, top_k, complexity, f, d_keys, d_dists, d_counts, d_stats, st, nullptr)
                    : leann_internal_search_plain(h, d_q, nq, top_k, complexity, f, d_keys, d_dists, d_counts, d_stats, st);
    if (rc) return fail(rc);
    std::vector<uint32_t> hstats(ns * nq * 4);
    if (zero_copy) {
        if (hipStreamSynchronize(st) != hipSuccess) {
            leann_set_error("search: device error: %s", hipGetErrorString(hipGetLastError()));
            return fail(LEANN_ERR_DEVICE);
        }
        memcpy(keys, w->pin + o_keys, no * 8);
        memcpy(dists, w->pin + o_dists, no * 4);
        memcpy(counts, w->pin + o_counts, nq * 4);
        memcpy(hstats.data(), w->pin + o_stats, nq * 16);
    } else
    if (hipMemcpyAsync(keys, w->d_keys, no * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(dists, w->d_dists, no * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(counts, w->d_counts, nq * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(hstats.data(), w->d_stats, ns * nq * 16, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        leann_set_error("search: device error: %s", hipGetErrorString(hipGetLastError()));
        return fail(LEANN_ERR_DEVICE);
    }
    size_t n_lost = 0;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        const GraphView &gv = h->sharded ? leann_internal_sharded_shard(h->sharded, 0)->g : h->g; // (shards share one configuration)
        const leann_backend *const h0 = h->sharded ? leann_internal_sharded_shard(h->sharded, 0) : h;
        const NarrowRows *const t = leann_internal_narrow(h0->row_type);
        const size_t elem_bytes = t ? t->elem_bytes : 4;
        for (size_t i = 0; i < ns * nq; i++) {
            h->stats.n_dist_evals += hstats[i * 4 + 0];
            h->stats.n_hops_base += hstats[i * 4 + 1];
            h->stats.n_hops_upper += hstats[i * 4 + 2];
            h->stats.n_table_overflow += hstats[i * 4 + 3] ? 1 : 0;
            n_lost += hstats[i * 4 + 3] == 3;
            h->stats.algorithmic_bytes += (uint64_t)hstats[i * 4 + 0] * (gv.feat_h ? (gv.norms ? 2 * (size_t)gv.feat_h + 4 : (size_t)gv.row_bytes) : d * elem_bytes) + (uint64_t)hstats[i * 4 + 1] * gv.M0 * 4 +
                                          (uint64_t)hstats[i * 4 + 2] * gv.M * 4;
        }
        h->stats.n_queries += nq;
        h->free_ws.push_back(std::move(w));
    }
    if (n_lost) { // search.cuh: the last visited-table level filled up (not reachable with the pools ensure_gpool sizes)
        leann_set_error("search: %zu of %zu queries ran out of visited-set space at complexity %zu; lower the complexity", n_lost, nq,
                        std::max(leann_internal_effective_complexity(h, complexity), top_k));
        return LEANN_ERR_OVERFLOW;
    }
    return LEANN_OK;
}

static int search_filtered_batch_host(const leann_backend *hc, const float *queries, size_t nq, size_t top_k, size_t complexity,
                                      const uint8_t *allow, size_t allow_stride, uint64_t *keys, float *dists, uint32_t *counts, int mode,
                                      const leann_filter *flt) {
    try { // std::bad_alloc and friends must not cross the C ABI (every host-pointer search entry point funnels through here)
        return search_filtered_batch_host_impl(hc, queries, nq, top_k, complexity, allow, allow_stride, keys, dists, counts, mode, flt);
    } catch (const std::exception &e) {
        leann_set_error("search: %s", e.what());
        return LEANN_ERR_DEVICE;
    }
}

// ---- request coalescing --------------------------------------------------------------
// The reference serves one query per call from many threads (cli/serve.rs:289-292).  One query is one
// workgroup: ~1 ms of latency and 1/1000 of the chip.  With coalescing enabled on a handle, concurrent
// leann_backend_search callers are gathered for up to `wait_us` (or `max_batch` queries) and answered by ONE
// batched launch, transparently to the callers — the Rust server needs no change.
struct PendingQuery {
    const float *q;
    size_t k, ef;
    uint64_t *keys;
    float *dists;
    size_t *n_out;
    int rc = 0;
    bool done = false, answered = false;
    std::string err;
};
struct Coalescer {
    leann_backend *h = nullptr;
    uint32_t wait_us = 200, max_batch = 4096;
    std::mutex mu;
    std::condition_variable cv_submit, cv_done;
    std::vector<PendingQuery *> queue;
    std::thread th;
    bool stop = false;
    uint64_t n_launches = 0, n_queries = 0;
    size_t recent_callers = 0; // size of the previous batch + the queue behind it when it completed

    void run() {
        (void)hipSetDevice(h->device);
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            // The window ends early once as many callers as were seen lately (the previous batch + what had queued up behind it) are
            // waiting again.  A batch of this size costs about what one query costs (the walk is latency-bound), so one full herd beats
            // two alternating halves (8 threads: 17 k against 12 k queries/s) and firing at once on whatever is there (ditto).
            cv_submit.wait(lk, [&] { return stop || !queue.empty(); });
            if (stop && queue.empty()) return;
            const size_t fire_at = std::min<size_t>(max_batch, std::max<size_t>(1, recent_callers));
            auto deadline = std::chrono::steady_clock::now() + std::chrono::microseconds(wait_us);
            cv_submit.wait_until(lk, deadline, [&] { return stop || queue.size() >= fire_at; });
            std::vector<PendingQuery *> batch;
            batch.swap(queue);
            lk.unlock();
            // one launch per distinct (top_k, complexity)
            std::map<std::pair<size_t, size_t>, std::vector<PendingQuery *>> groups;
            for (auto *p : batch) groups[{p->k, p->ef}].push_back(p);
            const size_t d = h->g.d;
            try { // (an allocation failure in here must reach the callers as an error, not end the process from a library thread)
            for (auto &kv : groups) {
                auto &g = kv.second;
                const size_t nq = g.size(), k = kv.first.first;
                std::vector<float> Q(nq * d);
                for (size_t i = 0; i < nq; i++) memcpy(Q.data() + i * d, g[i]->q, d * 4);
                std::vector<uint64_t> keys(nq * std::max<size_t>(k, 1));
                std::vector<float> dists(nq * std::max<size_t>(k, 1));
                std::vector<uint32_t> counts(nq);
                int rc = leann_backend_search_batch(h, Q.data(), nq, k, kv.first.second, keys.data(), dists.data(), counts.data());
                std::string err = rc ? leann_last_error() : "";
                for (size_t i = 0; i < nq; i++) {
                    if (!rc) {
                        memcpy(g[i]->keys, keys.data() + i * k, counts[i] * 8);
                        memcpy(g[i]->dists, dists.data() + i * k, counts[i] * 4);
                        *g[i]->n_out = counts[i];
                    }
                    g[i]->rc = rc;
                    g[i]->err = err;
                    g[i]->answered = true;
                }
                n_launches++;
                n_queries += nq;
            }
            } catch (const std::exception &e) {
                for (auto *p : batch)
                    if (!p->answered) { p->rc = LEANN_ERR_DEVICE; p->err = std::string("request coalescing: ") + e.what(); *p->n_out = 0; }
            }
            lk.lock();
            recent_callers = batch.size() + queue.size();
            for (auto *p : batch) p->done = true;
            cv_done.notify_all();
        }
    }
};

// Safe against searches in flight: the handle's coalescer is swapped out under h->mu, the lock is RELEASED, and only then is the old
// dispatcher stopped and joined (it drains its queue first; its launches take h->mu themselves).  Callers hold a shared_ptr, so the
// object outlives every waiter; a caller that arrives after `stop` answers its query directly.
static std::shared_ptr<Coalescer> make_coalescer(leann_backend *h, uint32_t wait_us, uint32_t max_batch) {
    auto fresh = std::make_shared<Coalescer>();
    fresh->h = h;
    fresh->wait_us = wait_us;
    fresh->max_batch = max_batch ? max_batch : 4096;
    Coalescer *c = fresh.get();
    fresh->th = std::thread([c] { c->run(); });
    return fresh;
}
static void retire_coalescer(std::shared_ptr<Coalescer> old) {
    if (!old) return;
    { std::lock_guard<std::mutex> l2(old->mu); old->stop = true; }
    old->cv_submit.notify_all();
    old->th.join();
}
extern "C" int leann_backend_set_coalescing(leann_backend *h, uint32_t wait_us, uint32_t max_batch) {
    if (!h) { leann_set_error("leann_backend_set_coalescing: null handle"); return LEANN_ERR_INVALID; }
    std::shared_ptr<Coalescer> fresh, old;
    const bool off = wait_us == 0 && max_batch == 0;
    if (!off) fresh = make_coalescer(h, wait_us, max_batch);
    {
        std::lock_guard<std::mutex> lk(h->mu);
        old.swap(h->coalescer);
        h->coalescer = fresh;
        h->coalesce_mode = off ? 2 : 1;
    }
    retire_coalescer(old);
    return LEANN_OK;
}
int leann_internal_copy_coalescing(const leann_backend *srcc, leann_backend *dst) {
    leann_backend *src = const_cast<leann_backend *>(srcc);
    int mode = 0;
    uint32_t wait_us = 0, max_batch = 0;
    {
        std::lock_guard<std::mutex> lk(src->mu);
        mode = src->coalesce_mode;
        if (mode == 1 && src->coalescer) { wait_us = src->coalescer->wait_us; max_batch = src->coalescer->max_batch; }
    }
    if (mode == 0) return LEANN_OK; // automatic: the default of a new handle
    return leann_backend_set_coalescing(dst, wait_us, max_batch); // (mode 2: (0, 0) switches it off)
}
// Automatic mode (the default; LEANN_COALESCE=off in the environment or leann_backend_set_coalescing(h, 0, 0) switch it off): the
// reference's server calls search from many threads without knowing about batches (cli/serve.rs:289-292).  The first caller that
// finds another single-query call in flight on the handle installs a dispatcher (50 us window or 64 queries for a query that arrives at an idle dispatcher; whatever
// queued up while a batch ran leaves at once) and queues behind it; a
// caller that is alone is answered directly, at the latency of one launch.
static std::shared_ptr<Coalescer> auto_coalescer(leann_backend *h) {
    if (leann_knobs().coalesce_off) return nullptr;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        if (h->coalesce_mode != 0) return h->coalescer;
        if (h->coalescer) return h->coalescer;
    }
    std::shared_ptr<Coalescer> fresh = make_coalescer(h, 50, 64), lost;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        if (h->coalesce_mode == 0 && !h->coalescer) { h->coalescer = fresh; return fresh; }
        lost = fresh; // somebody else installed one (or configured the handle) meanwhile
        fresh = h->coalescer;
    }
    retire_coalescer(lost);
    return fresh;
}
extern "C" int leann_backend_coalescing_stats(const leann_backend *hc, uint64_t *n_launches, uint64_t *n_queries) {
    leann_backend *h = const_cast<leann_backend *>(hc);
    std::shared_ptr<Coalescer> c;
    if (h) { std::lock_guard<std::mutex> lk(h->mu); c = h->coalescer; }
    if (!c) { leann_set_error("coalescing is not enabled on this handle"); return LEANN_ERR_INVALID; }
    std::lock_guard<std::mutex> l2(c->mu);
    if (n_launches) *n_launches = c->n_launches;
    if (n_queries) *n_queries = c->n_queries;
    return LEANN_OK;
}

extern "C" int leann_backend_search(const leann_backend *hc, const float *query, size_t top_k, size_t complexity,
                                    uint64_t *keys, float *dists, size_t *n_out) {
    if (!n_out) { leann_set_error("leann_backend_search: n_out is null"); return LEANN_ERR_INVALID; }
    leann_backend *h = const_cast<leann_backend *>(hc);
    std::shared_ptr<Coalescer> c;
    struct InFlight { // single-query calls on this handle right now (automatic coalescing)
        std::atomic<int> *a;
        int before;
        explicit InFlight(std::atomic<int> *p) : a(p), before(p ? p->fetch_add(1) : 0) {}
        ~InFlight() { if (a) a->fetch_sub(1); }
    } inflight(h ? &h->singles_in_flight : nullptr);
    if (h && query && keys && dists && top_k > 0 && h->g.n > 0) {
        int mode;
        { std::lock_guard<std::mutex> lk(h->mu); c = h->coalescer; mode = h->coalesce_mode; }
        if (!c && mode == 0 && inflight.before > 0) c = auto_coalescer(h);
    }
    if (c) {
        PendingQuery p{query, top_k, complexity, keys, dists, n_out};
        std::unique_lock<std::mutex> lk(c->mu);
        if (!c->stop) { // a stopped dispatcher takes no new work: fall through to the direct call
            c->queue.push_back(&p);
            c->cv_submit.notify_one();
            c->cv_done.wait(lk, [&] { return p.done; });
            if (p.rc) leann_set_error("%s", p.err.c_str());
            return p.rc;
        }
    }
    uint32_t cnt = 0;
    int rc = leann_backend_search_batch(h, query, 1, top_k, complexity, keys, dists, &cnt);
    *n_out = cnt;
    return rc;
}

// One filtered query (host bitmap of ceil(len/8) bytes, uploaded with the call; callers with a recurring filter keep the
// bitmap in HBM and use the *_device entry point).  Not coalesced.
extern "C" int leann_backend_search_filtered(const leann_backend *hc, const float *query, size_t top_k, size_t complexity,
                                             const uint8_t *allow, uint64_t *keys, float *dists, size_t *n_out) {
    if (!n_out) { leann_set_error("leann_backend_search_filtered: n_out is null"); return LEANN_ERR_INVALID; }
    if (!allow) return leann_backend_search(hc, query, top_k, complexity, keys, dists, n_out);
    uint32_t cnt = 0;
    int rc = leann_backend_search_filtered_batch(hc, query, 1, top_k, complexity, allow, 0, keys, dists, &cnt);
    *n_out = cnt;
    return rc;
}

extern "C" int leann_backend_from_arrays(int backend, const float *vectors, size_t n, size_t dims, uint32_t M,
                                         uint32_t M0, uint32_t max_level, uint32_t entry, const uint8_t *levels,
                                         const uint32_t *upper_off, const uint32_t *adj0, const uint32_t *adjU,
                                         size_t n_upper_lists, int device, uint64_t key_offset, leann_backend **out) {
    try {
        return leann_internal_from_host(backend, n, dims, M, M0, max_level, entry, levels, upper_off, adj0, adjU, n_upper_lists, vectors,
                                        nullptr, 0, 0, nullptr, device, key_offset, out);
    } catch (const std::exception &e) {
        leann_set_error("leann_backend_from_arrays: %s", e.what());
        return LEANN_ERR_IO;
    }
}

// A composite (sharded) handle holds G graphs, so graph_info / graph_export / feature_rows_export apply per shard: the sub-index of a
// shard is an ordinary handle (borrowed: it lives as long as the composite one; keys it returns are global positions).
extern "C" size_t leann_backend_shard_count(const leann_backend *h) { return h && h->sharded ? leann_internal_sharded_count(h->sharded) : 0; }
extern "C" int leann_backend_shard(const leann_backend *h, size_t g, leann_backend **out) {
    if (!h || !out) { leann_set_error("leann_backend_shard: null argument"); return LEANN_ERR_INVALID; }
    *out = nullptr;
    if (!h->sharded || g >= leann_internal_sharded_count(h->sharded) || !leann_internal_sharded_shard(h->sharded, g)) {
        leann_set_error("leann_backend_shard: %s", h->sharded ? "no such shard" : "not a sharded handle");
        return LEANN_ERR_INVALID;
    }
    *out = leann_internal_sharded_shard(h->sharded, g);
    return LEANN_OK;
}

extern "C" int leann_backend_graph_info(const leann_backend *h, uint64_t *info) {
    if (!h || !info) { leann_set_error("leann_backend_graph_info: null argument"); return LEANN_ERR_INVALID; }
    info[0] = h->g.n; info[1] = h->g.d; info[2] = h->g.ld; info[3] = h->g.M; info[4] = h->g.M0;
    info[5] = h->g.max_level; info[6] = h->g.entry; info[7] = h->n_upper_lists;
    return LEANN_OK;
}
extern "C" int leann_backend_graph_export(const leann_backend *h, uint8_t *levels, uint32_t *upper_off, uint32_t *adj0,
                                          uint32_t *adjU, float *vectors) {
    if (!h) { leann_set_error("leann_backend_graph_export: null handle"); return LEANN_ERR_INVALID; }
    NOT_ON_SHARDED(h, "graph export");
    HIP_CHECK_RET(hipSetDevice(h->device));
    HIP_CHECK_RET(hipDeviceSynchronize());
    const size_t n = h->g.n;
    if (n == 0) return LEANN_OK;
    if (levels) HIP_CHECK_RET(hipMemcpy(levels, h->store.levels, n, hipMemcpyDeviceToHost));
    if (upper_off) HIP_CHECK_RET(hipMemcpy(upper_off, h->g.upper_off, n * 4, hipMemcpyDeviceToHost));
    if (adj0) HIP_CHECK_RET(hipMemcpy(adj0, h->g.adj0, n * h->g.M0 * 4, hipMemcpyDeviceToHost));
    if (adjU && h->n_upper_lists)
        HIP_CHECK_RET(hipMemcpy(adjU, h->g.adjU, h->n_upper_lists * h->g.M * 4, hipMemcpyDeviceToHost));
    if (vectors && h->g.feat_h) { leann_set_error("graph_export: a recompute-on index holds no vectors"); return LEANN_ERR_UNSUPPORTED; }
    if (const NarrowRows *t = vectors ? leann_internal_narrow(h->row_type) : nullptr) {
        // The widened rows: exact.  The narrow rows, e = elem_bytes each, land at the END of the caller's own buffer — e n d bytes of
        // 4 n d — and are widened in place, front to back: element i is written at bytes 4 i .. 4 i + 3 and read from bytes
        // (4 - e) n d + e i onward, which no earlier write has reached: 4 i + 4 <= (4 - e) n d + e i + e  <=>  (4 - e)(i + 1) <=
        // (4 - e) n d, true for every i < n d.
        const size_t d = h->g.d, nd = n * d;
        unsigned char *base = reinterpret_cast<unsigned char *>(vectors), *narrow = base + (4 - t->elem_bytes) * nd;
        try { // (the device-to-host staging slab is a std::vector)
            if (int rc = leann_internal_narrow_to_host(h, 0, n, narrow)) return rc;
        } catch (const std::exception &e) {
            leann_set_error("leann_backend_graph_export: %s", e.what());
            return LEANN_ERR_IO;
        }
        t->widen(narrow, nd, d, h->i8_exps.data(), base);
        return LEANN_OK;
    }
    if (vectors)
        HIP_CHECK_RET(hipMemcpy2D(vectors, (size_t)h->g.d * 4, h->g.X, (size_t)h->g.ld * 4, (size_t)h->g.d * 4, n,
                                  hipMemcpyDeviceToHost));
    return LEANN_OK;
}

