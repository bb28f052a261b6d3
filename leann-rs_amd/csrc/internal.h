// internal.h — structs and functions shared by the .hip files (not part of the C ABI).  Every leann_internal_* function is declared
// once, here (the four allocation functions: device_mem.h; the narrow row store: narrow_rows.h, included below).  Whatever a handle
// holds on its device is a DeviceBuf member of leann_backend / GraphStore, or a ScratchLease: `delete` frees it, nothing is freed by hand.
#pragma once
#include "search.cuh"
#include "device_mem.h"
#include "topk_plan.h"
#include "../../include/leann_backend.h"
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

struct Workspace { // staging of the host-pointer API; one per concurrent caller
    DeviceBuf<float> d_q, d_dists;
    DeviceBuf<uint64_t> d_keys;
    DeviceBuf<uint32_t> d_counts, d_stats;
    DeviceBuf<uint8_t> d_allow; // filtered searches: staged allow-bitmap(s)
    // small calls (a single query is the reference's own call, traits.rs:16-21): one block of pinned, device-mapped host memory
    // {queries | keys | dists | counts | stats}: the kernels read the queries from it and write the results into it, so the call
    // is kernel launches + one stream synchronisation, with no copy engine in between
    unsigned char *pin = nullptr;
    size_t cap_pin = 0;
    hipStream_t stream = nullptr;
    ~Workspace(); // api.hip: the pinned block and the stream
};

// Environment knobs of the SEARCH path.  The environment is read ONCE — when the library is first used — into this struct; a search
// call never calls getenv (it used to, five times per call: a 50-us call paid five environment scans, and getenv racing a setenv in a
// multi-threaded Rust host is undefined behaviour).  Tests that flip a diagnostic knob on a live handle call leann_debug_reload_env().
struct LeannKnobs {
    int hash_bits = 0;      // LEANN_DEBUG_HASH_BITS: force the LDS visited table to 2^bits slots (6..15; 0 = automatic)
    int nw = 0;             // LEANN_DEBUG_NW: waves per query (0 = by batch size)
    int gpool_bits = 0, gpool2_bits = 0; // LEANN_DEBUG_GPOOL_BITS / _GPOOL2_BITS (0 = default sizes)
    int row_screen = 1;              // LEANN_ROW_SCREEN: what handles made from now on do about the row screen (planes.hip): 0 = off, no
                                     // split planes (A/B runs); 1 = automatic (default): planes for indexes whose rows outgrow the caches;
                                     // 2 (LEANN_ROW_SCREEN=1) = planes whatever the size
    bool no_feat256 = false, no_zero_copy = false, no_emit = false, fused_v1 = false, no_list = false, no_tiled = false;
    bool force_remote = false;       // LEANN_DEBUG_FORCE_REMOTE: sharded searches treat EVERY shard as if it sat on another device (staging
                                     // buffers + peer copies, with source = destination device) — exercises that branch on a one-GPU box
    bool coalesce_off = false;       // LEANN_COALESCE=off|0
    bool hnsw_reference_ef = false;  // LEANN_HNSW_REFERENCE_EF=1: HNSW handles opened from now on search with ef = 64 whatever
                                     // `complexity` says, as the reference does (hnsw.rs:49 expansion_search: 64, :83 _complexity unused)
    unsigned long long stamp_buf = 0; // LEANN_STAMP_BUF (diagnostic builds only)
    bool meta_device = true;         // LEANN_META_DEVICE=0: a host that evaluates metadata filters on the device (the C++ IndexSearcher)
                                     // takes its per-passage loop instead (A/B runs; leann_meta_device_enabled)
    unsigned long long meta_batch_bytes = 0; // LEANN_DEBUG_META_BATCH_BYTES: the bitmap scratch leann_backend_search_meta_batch* holds at a
                                     // time instead of 1 GiB, so that small tests cross chunk boundaries (0 = unset)
};
const LeannKnobs &leann_knobs();
extern "C" void leann_debug_reload_env(void);
extern std::atomic<uint64_t> leann_internal_device_blocks; // api.hip: blocks owned through DeviceBuf and ScratchLease (leann_debug_device_blocks)

// What a plain handle's graph owns on its device.  GraphView (search.cuh) is the kernels' read-only view of it: its pointers are set
// from these members next to the allocation that fills them.  Builder and graph repair write through the members.
struct GraphStore {
    DeviceBuf<unsigned char> rows; // f32 rows, a narrow type's store or feature rows; EMPTY = g.X names the caller's rows (borrowed)
    DeviceBuf<float> norms;        // the split feat_h == 256 layout's norms, or int8 rows' column scales
    DeviceBuf<uint32_t> adj0, adjU, upper_off;
    DeviceBuf<uint8_t> levels;
};
struct Coalescer;
struct leann_sharded;
inline std::atomic<uint64_t> leann_internal_handle_serial{0};
struct leann_backend {
    const uint64_t serial = ++leann_internal_handle_serial; // never reused: a registered filter names the handle it was made for by it
    leann_sharded *sharded = nullptr; // composite handle (shard.hip): searches fan out to the sub-indexes; g holds only n and d
    int kind = LEANN_BACKEND_HNSW, device = 0;
    GraphView g{};
    GraphStore store; // (a composite handle's stays empty: the sub-indexes own the device memory)
    uint64_t key_offset = 0;
    uint32_t efc = 64;
    float alpha = 1.2f;
    uint32_t fixed_ef = leann_knobs().hnsw_reference_ef ? 64u : 0u; // reference-exact mode, latched when the handle is made (HNSW only)
    bool nav_levels = false; // Vamana built with entry layers (build.hip); searches need nothing but g.max_level / g.entry
    uint64_t n_upper_lists = 0;
    std::mutex mu;
    std::vector<std::unique_ptr<Workspace>> free_ws; // host-pointer API: one per concurrent caller
    // pooled HBM visited tables (search.cuh): shared by every stream, handed out by in-kernel locks
    DeviceBuf<unsigned long long> gpool, gpool2;
    DeviceBuf<uint32_t> gpool_lock, gpool2_lock;
    uint32_t *gpool_ctr = nullptr; // inside gpool_lock
    uint32_t gpool_bits = GPOOL_BITS, gpool_tables = GPOOL_TABLES, gpool2_bits = 0, gpool2_tables = 0;
    leann_search_stats stats{};
    // recompute-on graph mode (g.feat_h != 0): encoder weights as f32 [feat_h x dims] for the query projection and
    // per-stream scratch for the projected queries
    DeviceBuf<float> Wf32;
    std::map<hipStream_t, DeviceBuf<float>> proj_scratch;
    std::shared_ptr<Coalescer> coalescer; // optional request coalescing for single-query callers (api.hip); swapped under `mu`
    // 0 = automatic (default): a leann_backend_search caller that finds another one in flight goes through a dispatcher created on the
    // spot, a lone caller is answered directly; 1 = configured by leann_backend_set_coalescing; 2 = switched off by it
    int coalesce_mode = 0;
    std::atomic<int> singles_in_flight{0};
    // removals (consolidate.hip): positions are never renumbered; a removed position keeps its row and is masked out of every search.
    // removed: host bitmap (bit set = removed), empty until the first removal.  d_live: its complement on the device (padding bits 0),
    // null until the first removal — a handle without removals takes none of the code paths below.  n_pending: removed positions a live
    // list still names (0 after leann_backend_consolidate: unfiltered walks then run the plain kernel again).  removal_epoch counts
    // the leann_backend_remove calls that removed something; a registered filter remembers the epoch it was made in.
    std::vector<uint8_t> removed;
    DeviceBuf<uint8_t> d_live;
    size_t n_removed = 0, n_pending = 0;
    uint64_t removal_epoch = 0;
    uint32_t two_stage = 1; // Vamana: the RobustPrune form the build used (LEANN_VAMANA_TWO_STAGE when the handle was made)
    std::map<hipStream_t, DeviceBuf<uint8_t>> live_scratch; // per stream: live AND the caller's bitmap(s)
    // Row screen (planes.hip, row_screen.h): the f32 rows a second time as two planes of 16-bit halves, [n x ldp] u16 each, owned by the
    // handle whoever owns X; planes_src / planes_n / planes_ld name the rows they were cut from.  screen_ctr: device totals
    // {rows ruled out, rows read in full}.  row_screen: 0 off, 1 automatic, 2 on whatever the size (LeannKnobs::row_screen when the
    // handle is made; leann_backend_set_row_screen switches between 0 and 2).
    DeviceBuf<uint16_t> x_hi, x_lo;
    uint32_t ldp = 0, planes_ld = 0;
    const float *planes_src = nullptr;
    uint64_t planes_n = 0;
    DeviceBuf<unsigned long long> screen_ctr;
    std::atomic<int> row_screen{leann_knobs().row_screen};
    // Row type: LEANN_ROWS_F32, or a narrow type (narrow_rows.h: LEANN_ROWS_BF16, LEANN_ROWS_I8) — then g.X names the handle's own store in
    // that type's layout and no f32 rows exist: every path that reads g.X as f32 checks this first.  (A recompute-on handle reports
    // LEANN_ROWS_FEATURES through leann_backend_row_type; here it is g.feat_h != 0 as before.)  i8_exps: int8 rows' column exponents e_j
    // [g.d], on the host; their scales 2^-e_j are g.norms (store.norms), f32 [g.ld].
    int row_type = LEANN_ROWS_F32;
    std::vector<int8_t> i8_exps;
};
#include "narrow_rows.h"
inline bool leann_internal_bf16(const leann_backend *h) { return h->row_type == LEANN_ROWS_BF16; }
inline bool leann_internal_i8(const leann_backend *h) { return h->row_type == LEANN_ROWS_I8; }
// the handle stores its vectors in a narrow type: no f32 rows exist for a scan, the builder or the graph repair to read
inline bool leann_internal_narrow_rows(const leann_backend *h) { return leann_internal_narrow(h->row_type) != nullptr; }
inline const char *leann_internal_row_name(const leann_backend *h) {
    const NarrowRows *t = leann_internal_narrow(h->row_type);
    return t ? t->name : "f32";
}
int leann_internal_check_build_args(int backend, size_t graph_degree, size_t complexity); // build.hip: backend and list lengths
// api.hip: dst takes src's coalescing configuration (automatic, configured with src's window and batch, or switched off)
int leann_internal_copy_coalescing(const leann_backend *src, leann_backend *dst);
// build.hip: leann_backend_build_device (rows borrowed) without cutting the row screen's planes
int leann_internal_build_device_no_planes(int backend, const float *d_vectors, size_t n, size_t dims, size_t ld, size_t graph_degree,
                                          size_t complexity, int device, uint64_t key_offset, leann_backend **out);
// Kernel tables (api.hip; search_bf16.hip for the bf16 rows' kernels): one row per compiled traversal kernel, keyed by the fields of a
// SearchPlan (search_plan.h) that name it.  A plan without a row is an error, never a neighbouring kernel.
using SearchKernel = void (*)(GraphView, SearchArgs); // every traversal kernel of search.cuh and search_bf16.hip
struct SearchKernelRow {
    int family, T, R, NW;
    bool wide, filtered, build;
    SearchKernel kernel;
};
template <size_t N>
inline int leann_internal_find_kernel(const SearchKernelRow (&rows)[N], const SearchPlan &p, SearchKernel *out) {
    for (const SearchKernelRow &r : rows)
        if (r.family == p.family && r.T == p.T && r.R == p.R && r.NW == p.NW && r.wide == p.wide && r.filtered == p.filtered && r.build == p.build) {
            *out = r.kernel;
            return LEANN_OK;
        }
    char name[96];
    search_plan_name(p, name, sizeof name);
    leann_set_error("search: no kernel %s is compiled", name);
    return LEANN_ERR_INVALID;
}
int leann_internal_bf16_kernel(const GraphView &g, const SearchPlan &p, SearchKernel *out); // search_bf16.hip: checks the row store too
int leann_internal_i8_kernel(const GraphView &g, const SearchPlan &p, SearchKernel *out);   // search_i8.hip: the same for int8 rows
// the one launch of a traversal kernel (api.hip): > 64 KiB of LDS is asked for first; grid = a.nq workgroups of p.NW waves
int launch_plan(SearchKernel kernel, const SearchPlan &p, const GraphView &g, const SearchArgs &a, hipStream_t st);
bool leann_internal_screen_shape(const GraphView &g);      // the row widths and list lengths the screen kernel is compiled for
void leann_internal_sync_planes(leann_backend *h);          // (re)build the planes of a plain handle; logs and returns on failure
bool leann_internal_planes_ready(const leann_backend *h);   // planes present and cut from the rows h->g names now
void leann_internal_free_planes(leann_backend *h);           // logs what the screen did, then drops the planes
// Removals (consolidate.hip).  leann_internal_live_allow: the bitmap a search on `h` has to run under — the caller's (may be null)
// ANDed with the live mask into the stream's scratch; *out = d_allow unchanged for a handle without removals.  `walk`: the search is
// the graph walk, which needs no mask of its own once no live list names a removed position.  One caller: leann_internal_search_plain.
int leann_internal_live_allow(leann_backend *h, const uint8_t *d_allow, size_t allow_stride, size_t nq, bool walk, hipStream_t st,
                              const uint8_t **out, size_t *out_stride);
int leann_internal_set_removed(leann_backend *h, const uint8_t *bitmap, size_t n_removed); // adopt a bitmap (open): device mask + n_pending
std::string leann_internal_tombstone_file(const std::string &index_file);
int leann_internal_tombstones_save(const leann_backend *h, const std::string &index_file); // writes the sidecar, or removes a stale one
int leann_internal_tombstones_load(leann_backend *h, const std::string &index_file);

// LEANN_LOG=error|warn|info|debug (default warn) -> stderr, "LEVEL leann_hip: message" (the reference logs through tracing, cli/mod.rs:38-43)
enum { LEANN_LOG_ERROR = 0, LEANN_LOG_WARN = 1, LEANN_LOG_INFO = 2, LEANN_LOG_DEBUG = 3 };
void leann_log(int level, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
bool leann_log_enabled(int level); // for callers whose message costs something to gather
// ---- making a handle (handle.hip): what every way in shares ------------------------------------------------------------------------
// src rows [rows x src_ld] (`dims` floats of each are data), on the host (`from_host`) or on the current device, into dst, f32
// [rows x dst_ld] on the current device, padding columns zero.  A plain copy when both pitches equal dims, else one hipMemcpy2D,
// behind a zero fill of dst only when dst_ld != dims.  The caller words the message.
hipError_t leann_internal_stage_rows(float *dst, size_t dst_ld, const float *src, size_t src_ld, size_t dims, size_t rows, bool from_host);
// `rows` unpadded f32 rows of `dims` floats from `byte_offset` of a file -> *out (empty), [rows x dims rounded up to 4] on `device`,
// which is checked and selected once the file is open; in slabs of 256 MiB of file rows.  LEANN_ERR_NOT_FOUND: the file cannot be
// opened or positioned; LEANN_ERR_IO: reading or uploading failed, *out is empty again — for these two the caller words the message.
int leann_internal_rows_from_file(const std::string &path, uint64_t byte_offset, size_t rows, size_t dims, int device, DeviceBuf<float> *out);
// The graph of an index that came without one this library can read: built on `rows` (f32 [n x dims rounded up to 4] on `device`)
// with degree 32 (HNSW) / 64 (DiskANN) and complexity 128, or LEANN_REBUILD_DEGREE / LEANN_REBUILD_COMPLEXITY.  *out owns the rows
// (on failure they stay the caller's) and is saved as `cache_path`; a cache that cannot be written is a warning.
int leann_internal_rebuild_from_rows(int backend, DeviceBuf<float> &&rows, size_t n, size_t dims, int device, uint64_t key_offset,
                                     const std::string &cache_path, leann_backend **out);
int leann_internal_use_device0(); // the file builders' device: selects device 0, or LEANN_ERR_DEVICE and "no HIP device visible ..."
// The owning pointer of a handle under construction: an early return closes it (leann_backend_close frees whatever it holds by then).
struct HandleClose { void operator()(leann_backend *h) const { leann_backend_close(h); } };
using HandlePtr = std::unique_ptr<leann_backend, HandleClose>;
// A new handle with src's kind, device, key_offset, build parameters (below), row_type and g — every device pointer of g null, and
// nothing else of src's (no memory, removals, planes or coalescing).  The caller changes only what it means to change.
HandlePtr leann_internal_new_like(const leann_backend *src);
void leann_internal_take_build_params(leann_backend *dst, const leann_backend *src); // efc, alpha, two_stage, nav_levels, fixed_ef
// dst, over n_new >= src->g.n positions of which the first src->g.n are src's, takes src's removals (snapshot under src->mu): the
// further positions are live, the live mask is uploaded and n_pending counted on the device.  Nothing to do for a src without removals.
int leann_internal_carry_removals(const leann_backend *src, leann_backend *dst, size_t n_new);
// uo[i] = number of upper lists in front of node i (the exclusive prefix sum of the level table); returns their total
uint64_t leann_internal_upper_offsets(const uint8_t *levels, size_t n, uint32_t *uo);
// adj0 [max(n, 1) x M0], adjU [max(n_upper_lists, 1) x M] filled with LEANN_EMPTY, upper_off and levels [max(n, 1)] into h->store
// (g.n, M, M0 set; h's device current); binds the view and sets h->n_upper_lists.  A level array that is there already is kept
// (compact.hip gathers the levels first: they say how many upper lists there are).
int leann_internal_alloc_graph_lists(leann_backend *h, uint64_t n_upper_lists);
// h owns `rows` from here on and g.X names them: the one place store.rows and g.X are set together.  A handle that was built on
// borrowed rows (leann_backend_build_device with take_copy = 0) borrows them until this call.
template <typename T>
inline void leann_internal_own_rows(leann_backend *h, DeviceBuf<T> &&rows) {
    h->store.rows = DeviceBuf<unsigned char>(std::move(rows));
    h->g.X = reinterpret_cast<const float *>(h->store.rows.p);
}
// host-side graph arrays -> device index; exactly one of `vectors` (f32 rows [n x dims]) and `feat_rows` (recompute-on rows
// [n x row_bytes] + Wf32 [feat_h x dims]) is given.  Validates every array against n before anything is uploaded.
int leann_internal_from_host(int backend, size_t n, size_t dims, uint32_t M, uint32_t M0, uint32_t max_level, uint32_t entry,
                             const uint8_t *levels, const uint32_t *upper_off, const uint32_t *adj0, const uint32_t *adjU,
                             size_t n_upper_lists, const float *vectors, const unsigned char *feat_rows, uint32_t feat_h, uint32_t row_bytes,
                             const float *Wf32, int device, uint64_t key_offset, leann_backend **out, int row_type = LEANN_ROWS_F32,
                             const NarrowSource *narrow = nullptr);
// ^ a narrow row_type (narrow_rows.h): the rows come as host f32 `vectors` or from one of `narrow`'s sources — an index file's rows in
//   the handle's own type, or device f32 rows (leann_backend_to_rows) — exactly one of the three, narrowed by the type's encode kernel.
int leann_internal_save_to(const leann_backend *h, const std::string &path);
int leann_internal_parse_device(const char *spec, int *device);
int leann_internal_check_device(int device); // api.hip: LEANN_ERR_DEVICE and the "no CPU fallback" message unless `device` is a visible one
// sharded handles (shard.hip)
bool leann_internal_spec_is_sharded(const char *spec);
int leann_internal_sharded_primary(const leann_sharded *s);
// indexfile.hip: open one file of this library's own format on `device`; *why says what was wrong with a file that is not one
int leann_internal_load_own_file(const std::string &path, int backend, size_t dims, int device, leann_backend **out, std::string *why);
int leann_internal_open_sharded_backend(const char *stem, int backend, size_t dims, const char *spec, leann_backend **out);
size_t leann_internal_sharded_count(const leann_sharded *s);
leann_backend *leann_internal_sharded_shard(const leann_sharded *s, size_t g);
// A filter registered on the device (leann_backend_filter_create): the bitmap, the ascending list of allowed positions and its length.
// On a composite handle: one sub-filter per shard (its slice of the bitmap, on the shard's device); n / n_allowed are the totals.
struct leann_filter {
    int device = 0;
    size_t n = 0, n_allowed = 0;
    DeviceBuf<uint8_t> d_allow;
    ScratchLease<uint32_t> d_list; // held for the filter's lifetime
    uint64_t epoch = 0;         // the handle's removal_epoch when the filter was made (its bitmap holds live positions only)
    uint64_t owner = 0;         // that handle's serial: a copy of it of the same length (leann_backend_append with n == 0) is another handle
    std::vector<leann_filter *> parts;
};
// api.hip: the two ends of registering a filter on a plain handle (leann_backend_filter_create uploads the bitmap in between,
// leann_backend_filter_create_meta evaluates it there).  _begin: h's device current, *out a filter with room for the bitmap.  _finish:
// epoch, owner, live mask, list of allowed positions; on failure f is deleted and *out stays null.
int leann_internal_filter_begin(const leann_backend *h, const char *who, leann_filter **out);
int leann_internal_filter_finish(const leann_backend *h, leann_filter *f, leann_filter **out);
// How one search call filters — the same description for every entry point, for a plain handle and for a composite one.
// Nothing set: no filter.  d_allow: a device bitmap over the handle's positions (a composite handle: GLOBAL positions on its first
// device, sliced per shard at byte boundaries); allow_stride == 0: one bitmap for the batch, else bytes from one query's to the next.
// registered: a leann_filter of this handle instead (a composite handle's holds one sub-filter per shard).  exact: scan the allowed
// rows instead of walking the graph.
struct SearchFilter {
    const uint8_t *d_allow = nullptr;
    size_t allow_stride = 0;
    const leann_filter *registered = nullptr;
    bool exact = false;
};
inline int leann_internal_check_allow_stride(const SearchFilter &f, size_t n) { // per-query bitmaps of n positions must not overlap
    if (f.d_allow && f.allow_stride && f.allow_stride < (n + 7) / 8) {
        leann_set_error("filtered search: allow_stride %zu is smaller than the %zu-byte bitmap", f.allow_stride, (n + 7) / 8);
        return LEANN_ERR_INVALID;
    }
    return LEANN_OK;
}
// THE search on a plain (non-sharded) handle — every entry point, and every shard of a composite handle, ends here (api.hip).  The
// caller has selected h's device; queries and outputs are device-accessible; d_stats [nq x 4] may be null.  Stream-ordered on `st`.
// (hidden: the library exports no name for it)
__attribute__((visibility("hidden"))) int leann_internal_search_plain(leann_backend *h, const float *d_queries, size_t nq, size_t top_k, size_t complexity, const SearchFilter &f,
                                uint64_t *d_keys, float *d_dists, uint32_t *d_counts, uint32_t *d_stats, hipStream_t st);
int leann_internal_sharded_search(leann_sharded *s, const float *d_queries, size_t nq, size_t top_k, size_t complexity, const SearchFilter &f,
                                  uint64_t *d_keys, float *d_dists, uint32_t *d_counts, uint32_t *d_stats, hipStream_t st, uint64_t *ticket);
int leann_internal_sharded_save(const leann_sharded *s, const char *index_path_stem);
uint64_t leann_internal_sharded_lo(const leann_sharded *s, size_t g);
int leann_internal_filtered_exact_list(const float *d_rows, size_t dims, size_t ld, const float *d_queries, size_t nq, size_t top_k,
                                       const uint32_t *d_list, size_t m, uint64_t key_offset, uint64_t *d_keys, float *d_dists,
                                       uint32_t *d_counts, hipStream_t st);
int leann_internal_filtered_exact(const float *d_rows, size_t n, size_t dims, size_t ld, const float *d_queries, size_t nq, size_t top_k,
                                  const uint8_t *d_allow, size_t allow_stride, uint64_t key_offset, uint64_t *d_keys, float *d_dists,
                                  uint32_t *d_counts, hipStream_t st);
// scan.hip: bitmap over n positions -> *list, the allowed positions ascending (left empty when there are none), *n_list; synchronises
// the stream once for the count.  The lease ends only once the stream that read the list is synchronised.
int leann_internal_compact_allow(const uint8_t *d_allow, size_t n, ScratchLease<uint32_t> *list, size_t *n_list, hipStream_t st);
int leann_internal_and_live_inplace(const leann_backend *h, uint8_t *d_bitmap);
// scan.hip: segment top-k of a score slab and the reduction of its winners (bm25.hip's segment fallback, and the select step below)
int leann_internal_topk_chunk(const float *S, size_t rows, size_t nq, uint32_t k, const uint8_t *allow, uint64_t pos0, uint64_t *cand,
                              size_t cand_len, size_t seg_off, hipStream_t st, size_t *segs_out, uint64_t *best);
int leann_internal_scan_finish_ex(uint64_t *candA, uint64_t *candB, size_t cand_len, size_t total_segs, size_t nq, uint32_t k,
                                  uint64_t key_offset, uint64_t *d_keys, float *d_scores, uint32_t *d_counts, hipStream_t st,
                                  const uint32_t *idx, int as_dist);
// scan.hip: k-way merge of per-shard results (shard.hip, the sharded recompute search)
int leann_internal_merge_strided(const void *keys, const void *dists, const void *counts, size_t kstride, size_t dstride, size_t cstride,
                                 size_t n_shards, size_t nq, size_t k_in, size_t k_out, int descending, uint64_t *d_out_keys,
                                 float *d_out_dists, uint32_t *d_out_counts, hipStream_t st);
extern "C" void leann_sharded_close(leann_sharded *s);

int leann_internal_launch_search(leann_backend *h, SearchArgs a, hipStream_t st);
size_t leann_internal_effective_complexity(const leann_backend *h, size_t complexity);

// Candidate emission of the exhaustive searches (recompute_fstat.cuh, scan.hip): instead of writing an nq x rows score slab for a
// separate top-k pass, a scoring kernel compares each score with the query's running k-th best (fixed for the launch) and appends
// the few survivors (~k * rows / rows_seen per query) to a per-query list; leann_internal_fold_candidates merges the lists into the
// running best-k (ascending keys ~orderable(score) << 32 | position), publishes the new thresholds and resets the counters.
struct CandEmit {
    const float *thr;      // [slots] score of the running k-th best per query (+inf: query slot unused); null = the kernel writes its slab
    uint32_t *cnt;         // [slots] survivors appended so far (may exceed cap: the list then overflowed)
    uint64_t *list;        // [slots x cap] keys
    uint32_t cap;
    const uint8_t *allow;  // optional early filter over positions (recompute.rs:66-71)
    uint64_t pos0;         // position of the launch's first row
};
int leann_internal_fold_candidates(const CandEmit &em, uint32_t k, uint32_t nq, uint32_t slots, uint64_t *best, uint32_t *d_overflow,
                                   hipStream_t st);
// The select step of an exhaustive top-k (scan.hip), shared by the exact scan and the recompute search.  The caller plans
// (topk_plan.h), owns the scratch the plan sizes and scores each chunk itself; a search reads
//     plan, acquire or grow, begin, per query tile and chunk { score with chunk_emit(c), select_chunk }, finish,
// once more on the slab schedule (emit = false) if finish reports an overflowed candidate list.
struct TopkRun {
    TopkPlan plan;
    float *S;                   // [q_tile x plan.slab_rows]
    uint64_t *candA, *candB;    // [nq x plan.cand_len]
    uint64_t *best;             // [nq x k]
    unsigned char *emit_block;  // [plan.emit_bytes]; unused (null) unless plan.emit
    size_t nq;
    uint32_t k;
    const uint8_t *allow;       // optional filter over positions
    hipStream_t st;
    hipEvent_t done;            // optional: recorded behind finish's last launch, before it waits (the recompute search's timing)
    // set by begin
    CandEmit em;
    uint32_t *d_overflow;
    size_t seg_off;
    // what chunk c's scoring launch is given: the emission block for an emitted chunk, none (the kernel writes S) for a slab chunk
    CandEmit chunk_emit(size_t c) const {
        CandEmit e = plan.slab_chunk(c) ? CandEmit{} : em;
        e.pos0 = plan.chunks[c].first;
        return e;
    }
};
int leann_internal_topk_begin(TopkRun &run);
// chunk c of the queries [q0, q0 + nqt), scored: segment top-k and running best-k of a slab chunk, then the fold when emitting
int leann_internal_topk_select_chunk(TopkRun &run, size_t c, size_t q0, uint32_t nqt);
// the answer (from best under emission, else from all segment winners); waits for the stream; *overflowed: repeat with emit = false
int leann_internal_topk_finish(TopkRun &run, uint64_t key_offset, const uint32_t *idx, int as_dist, uint64_t *d_keys, float *d_scores,
                               uint32_t *d_counts, bool *overflowed);
int leann_internal_score(const float *X, size_t rows, size_t dims, size_t ld, const float *d_queries, size_t nq, size_t ldq, float *S,
                         hipStream_t st);
size_t leann_internal_feat_file_row_bytes(const GraphView &g);
int leann_internal_feat_rows_to_host(const leann_backend *h, size_t r0, size_t rows, unsigned char *out);
std::string leann_internal_index_file(const char *stem, int backend);
std::string leann_internal_with_extension(const std::string &stem, const char *ext);
