/*
 * leann_backend.h — C ABI of the MI355X-native ANN search path that replaces leann-rs's
 * backend layer (src/backend) and the arithmetic of its recompute search (src/index/recompute.rs).
 *
 * Every entry point cites the reference interface it replaces (path:line in decisiongraph/leann-rs).
 * Plain pointers and sizes only; no torch / HIP types.  Thread-safety: `*_search*` are re-entrant
 * on one handle (BackendSearcher: Send + Sync, src/backend/traits.rs:11; concurrent callers at
 * src/cli/serve.rs:289-292); open/close/build are not.
 *
 * Return value: 0 on success, non-zero error code otherwise; the message is available from
 * leann_last_error() (thread-local), mirroring the anyhow::Result strings of the reference.
 *
 * Distances: dist = 1 - <q, x> (MetricKind::IP, src/backend/hnsw.rs:45; DistDot,
 * src/backend/diskann.rs:8,36), ascending, ties broken by lower key.  Keys are 0-based positions
 * in embedding order (src/backend/hnsw.rs:129), widened to u64 (src/backend/diskann.rs:58).
 */
#ifndef LEANN_BACKEND_H
#define LEANN_BACKEND_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct leann_backend leann_backend;

/* enum BackendType { Hnsw, DiskAnn }  — src/backend/mod.rs:15-19 */
enum { LEANN_BACKEND_HNSW = 0, LEANN_BACKEND_DISKANN = 1 };

enum {
    LEANN_OK = 0,
    LEANN_ERR_INVALID = 1,      /* bad argument */
    LEANN_ERR_NOT_FOUND = 2,    /* "Index file not found" hnsw.rs:34-40 / diskann.rs:26-32 */
    LEANN_ERR_FORMAT = 3,       /* FAISS / foreign format, hnsw.rs:24-32,57-69; compat.rs:15-38 */
    LEANN_ERR_DEVICE = 4,       /* HIP runtime / no GPU */
    LEANN_ERR_UNSUPPORTED = 5,  /* e.g. DiskANN incremental add, mod.rs:93-98 */
    LEANN_ERR_IO = 6,
    LEANN_ERR_OVERFLOW = 7      /* a query ran out of visited-set space (defensive; see leann_backend_search_batch_device) */
};

const char *leann_last_error(void);
const char *leann_version(void);

/* ---- BackendType::load_searcher(index_path, dimensions)  src/backend/mod.rs:23-45 -------------
 * `index_path_stem` is ".../documents.leann"; the backend derives "<stem minus .leann>.index"
 * (hnsw.rs:19) or ".diskann" (diskann.rs:22) itself.
 * `device_spec`: NULL / "" / "0" ... = one HIP device ordinal; a list or range ("0,1,2,3", "0-7"; the same ordinal repeated =
 * several shards on one device) opens the index SHARDED: the rows (from "<stem>.embeddings", else from this library's own index
 * file) are split into contiguous position ranges, one sub-index with its own graph per entry, and the returned handle fans every
 * search out to them and merges the per-shard lists by (dist, key) — see "sharded indexes" below.  The Rust side passes
 * std::env::var("LEANN_DEVICES") here.
 * Files: this library's own format ("LEANNGX1": graph + vectors, or graph + encoder inputs for a recompute-on index).  A usearch /
 * diskann-rs file written by stock leann-rs is not readable; when the directory also holds "<stem>.embeddings"
 * (src/index/embeddings.rs:21-153) the graph is rebuilt from it on the GPU and cached as "<stem>.gpu.index" / ".gpu.diskann".
 * Every file is validated (header against file length, every neighbour id / list offset against n) before it reaches the device. */
int leann_backend_open(const char *index_path_stem, int backend, size_t dims,
                       const char *device_spec, leann_backend **out);

/* ---- BackendSearcher::search(&self, query, top_k, complexity)  src/backend/traits.rs:16-21 ----
 * Caller allocates keys/dists[top_k]; the first *n_out are filled, best first; *n_out <= top_k
 * (short results allowed, src/index/searcher.rs:139-143).  ef = max(complexity, top_k)
 * (diskann.rs:54).  Unlike hnsw.rs:83 `complexity` is honoured for HNSW too; with LEANN_HNSW_REFERENCE_EF=1 in the environment
 * when the handle is made, an HNSW handle behaves like the reference instead: ef = max(64, top_k) whatever `complexity` says
 * (expansion_search: 64, hnsw.rs:49; `_complexity` unused, :83). */
int leann_backend_search(const leann_backend *h, const float *query, size_t top_k,
                         size_t complexity, uint64_t *keys, float *dists, size_t *n_out);

/* Additive: nq queries [nq x dims] row-major in one launch; equals nq single calls.
 * keys/dists are [nq x top_k] (unused tail: key = UINT64_MAX, dist = +inf), counts[nq]. */
int leann_backend_search_batch(const leann_backend *h, const float *queries, size_t nq,
                               size_t top_k, size_t complexity, uint64_t *keys, float *dists,
                               uint32_t *counts);

/* Additive: metadata-filtered search with the filter evaluated INSIDE the traversal,
 * replacing IndexSearcher's fetch_k = 5*top_k over-fetch + post-filter (src/index/searcher.rs:129-133,:190-194).
 * `allow` is a bitmap over positions (bit i&7 of byte i>>3 set = position i may be returned; positions are local to
 * the handle, i.e. key - key_offset), ceil(len/8) bytes; in the batch call query i uses allow + i*allow_stride
 * (allow_stride == 0: one bitmap for the whole batch).  The graph is walked exactly as by the unfiltered search
 * (disallowed nodes still route); the answer is the top_k best allowed positions among EVERY node whose distance
 * the level-0 walk evaluated (~30x the beam), best first.  allow == NULL: the unfiltered search. */
int leann_backend_search_filtered(const leann_backend *h, const float *query, size_t top_k,
                                  size_t complexity, const uint8_t *allow, uint64_t *keys,
                                  float *dists, size_t *n_out);
int leann_backend_search_filtered_batch(const leann_backend *h, const float *queries, size_t nq,
                                        size_t top_k, size_t complexity, const uint8_t *allow,
                                        size_t allow_stride, uint64_t *keys, float *dists,
                                        uint32_t *counts);

/* Additive: the same filter answered EXACTLY, for filters that allow only a small share of the rows (a graph walk finds
 * few allowed nodes then: 1 % allowed -> filtered recall@10 0.86 at complexity 256).  The bitmap is compacted into the
 * list of allowed positions and only those rows are scanned (f32 matrix cores, one k-ordered fmaf chain per pair, like
 * leann_scan_topk_device): top_k best allowed positions by distance 1 - <x, q>, ties to the lower position; cost is
 * proportional to the number of allowed rows, independent of the graph.  The host-side planner
 * (host/leann_host.hpp IndexSearcher) switches to it below 5 % allowed (single queries; ~1.5 % is the crossover in 16k-query batches).  Needs stored vectors. */
int leann_backend_search_filtered_exact_batch(const leann_backend *h, const float *queries, size_t nq,
                                              size_t top_k, const uint8_t *allow, size_t allow_stride,
                                              uint64_t *keys, float *dists, uint32_t *counts);

/* Additive: a filter registered on the device.  A server answers many queries under the same metadata filter; the calls above
 * re-send the N/8-byte bitmap and (exact path) re-compact it for every query.  leann_backend_filter_create uploads the bitmap
 * and builds the list of allowed positions once; leann_backend_search_filter_batch then answers nq queries under it.
 * mode: 0 = walk the graph with the filter inside (leann_backend_search_filtered), 1 = exact scan of the allowed rows
 * (leann_backend_search_filtered_exact_batch), 2 = choose: exact when the filter allows <= 5 % of the rows or <= 64k rows
 * (batches of <= 64 queries) / <= 1.5 % (larger batches) and the index stores vectors, the walk otherwise.  Results are those of
 * the corresponding call above, bit for bit.  Free the filter only when no search is using it. */
typedef struct leann_filter leann_filter;
int leann_backend_filter_create(const leann_backend *h, const uint8_t *allow, leann_filter **out);
size_t leann_backend_filter_count(const leann_filter *f); /* allowed positions */
void leann_backend_filter_free(leann_filter *f);
/* The registered bitmap in HBM, on the handle's device: *d_allow [ceil(*n / 8)] over *n positions (n: optional), already "valid AND
 * match AND live" (leann_backend_filter_create ANDs the live mask; for removals alone register an all-ones bitmap).  Borrowed: valid
 * until the filter is freed.  It is an ordinary allow-bitmap, e.g. for the leann_bm25_*_filtered calls.  The filter of a composite
 * handle holds one slice per shard and no whole bitmap: LEANN_ERR_UNSUPPORTED — pass the caller's own bitmap there. */
int leann_backend_filter_bitmap_device(const leann_filter *f, const uint8_t **d_allow, size_t *n);
int leann_backend_search_filter_batch(const leann_backend *h, const float *queries, size_t nq, size_t top_k,
                                      size_t complexity, const leann_filter *filter, int mode,
                                      uint64_t *keys, float *dists, uint32_t *counts);

/* Additive: request coalescing for servers that call leann_backend_search from many threads (one query per
 * call, src/cli/serve.rs:289-292).  Concurrent callers are gathered for up to wait_us microseconds (or
 * max_batch queries) and answered by one batched launch; results are identical.  (0, 0) disables.
 * Without this call a handle coalesces automatically: a leann_backend_search caller that finds another one in
 * flight queues behind a dispatcher (50 us or 64 queries, ending early once the callers of the previous round
 * are all waiting again) created at that moment, a lone caller is answered
 * directly.  LEANN_COALESCE=off in the environment switches the automatic mode off for the process. */
int leann_backend_set_coalescing(leann_backend *h, uint32_t wait_us, uint32_t max_batch);
int leann_backend_coalescing_stats(const leann_backend *h, uint64_t *n_launches, uint64_t *n_queries);

/* Row screen.  For an index of stored f32 rows of 513..768 or 1 025..1 536 floats per row (lists of at most 64 ids) the library keeps
 * the rows a second time, split into the upper and the lower 16 bits of every element (two planes, together the size of the rows:
 * +30.7 GB at 10M x 768).  Unfiltered batches of more than 640 queries read a neighbour's upper halves first and its lower halves
 * only if a proved lower bound on its distance does not already put it behind a full beam; ids, distances, counts and stats are
 * bit-identical either way.  On by default for indexes whose rows take 1 GiB or more (smaller ones gain too, about 1.4x on a 307 MB
 * index, but are left out so that the benchmark's whole-row roofline figure stays below the HBM peak on its quick workload: DESIGN.md
 * section 2); LEANN_ROW_SCREEN=0 in the environment makes handles without the planes, LEANN_ROW_SCREEN=1 with them at any size.
 * If the planes do not fit, a warning is logged (LEANN_LOG) and searches read whole rows.  enable = 0: search whole rows (the
 * planes stay); 1: screen, whatever the size (cuts the planes if the handle has none; call it with no search in flight).  Works on
 * composite handles.
 * leann_backend_row_screen_stats: running totals since the handle was made — out[0] rows ruled out on their upper halves alone,
 * out[1] rows read in full (summed over the shards of a composite handle); waits for the device. */
int leann_backend_set_row_screen(leann_backend *h, int enable);
int leann_backend_row_screen_stats(const leann_backend *h, uint64_t out[2]);

/* BackendSearcher::len  src/backend/traits.rs:24 */
size_t leann_backend_len(const leann_backend *h);
size_t leann_backend_dims(const leann_backend *h);
/* Drop of Box<dyn BackendSearcher> */
void leann_backend_close(leann_backend *h);

/* ---- BackendBuilder::build(embeddings, ids, index_path, dims, graph_degree, complexity)
 *      src/backend/mod.rs:55-79 -> hnsw.rs:96-139 / diskann.rs:70-105 ---------------------------
 * vectors: [n x dims] row-major host memory.  Writes "<stem>.index" / "<stem>.diskann".
 * graph_degree: HNSW M in [2, 64] (level-0 lists hold 2 M <= 128 ids), DiskANN R in [2, 128]; outside -> LEANN_ERR_INVALID
 * before any device work.  Lists of more than 64 ids take the wide kernels; the file layout is the same. */
int leann_backend_build(int backend, const float *vectors, size_t n, size_t dims,
                        size_t graph_degree, size_t complexity, const char *index_path_stem);
/* BackendBuilder::add_to_index(embeddings, index_path, dims, start_id)  mod.rs:82-100,
 * hnsw.rs:142-191: appends to the index on disk (the new rows continue the insertion from the loaded graph; cost
 * proportional to the rows added).  DiskANN -> LEANN_ERR_UNSUPPORTED with the reference's message. */
int leann_backend_add(int backend, const float *vectors, size_t n, size_t dims, size_t start_id,
                      const char *index_path_stem);

/* ---- removing passages (additive; the reference can only append: `leann update`) -------------------------------------------------
 * leann_backend_remove marks keys as removed.  Keys are global (key_offset included); positions are never renumbered — the id map
 * above this ABI is positional —, so leann_backend_len stays the number of POSITIONS and leann_backend_live_len counts the rest.  An
 * unknown key -> LEANN_ERR_INVALID naming it, and nothing is applied; a key that is already removed is ignored and not counted in
 * *n_removed (may be NULL).  From then on EVERY leann_backend_search* entry point excludes removed positions: the walks run the
 * filtered kernel under live AND the caller's bitmap (so an unfiltered search then has the filtered search's semantics: top-k among
 * the evaluated nodes), the exact paths compact live AND allow.  A leann_filter registered before a later removal is refused with
 * LEANN_ERR_INVALID ("filter predates a removal; register it again").
 * leann_backend_consolidate repairs the graph on the device: every live node that named a removed one is re-linked
 * through that node's neighbours (FreshDiskANN Alg. 4) and pruned by the rule the build used; lists of removed nodes are cleared and
 * a removed entry point is replaced.  Afterwards no live list names a removed position, unfiltered walks use the plain kernel again,
 * exact and filtered paths keep ANDing the live mask.  A recompute-on handle (no f32 rows to prune on) -> LEANN_ERR_UNSUPPORTED: its
 * removals stay tombstones answered by the filtered walk.  A one-process composite handle routes each key to the shard that owns its
 * range and consolidates every shard; the ranks of an RCCL group remove from / consolidate their own shard handles.
 * Like open / build, remove and consolidate are NOT concurrent with searches on the same handle.  A handle without removals takes
 * exactly the code paths it took before these calls existed.
 * leann_backend_removed_bitmap: bit i&7 of byte i>>3 set = position i is removed (ceil(len/8) bytes); *n_pending (may be NULL) =
 * removed positions that live lists still name — 0 after a consolidate.
 * Persistence: leann_backend_save writes the removals beside the index file as "<stem minus .leann>.tombstones" ("LEANNTB1", u64 n,
 * u64 removed, u64 n_pending, the bitmap) or deletes a stale one when nothing is removed; leann_backend_open reads and validates it
 * (length against n, popcount against the count, zero padding bits; LEANN_ERR_FORMAT otherwise); leann_backend_add extends it with
 * zero bits; sharded save / open carry one per shard file.  The sidecar's name drops the index file's extension, so an HNSW and a
 * DiskANN index under ONE stem would share it: keep one backend per stem.  The index file layout is unchanged (a DiskANN file built
 * with the one-stage prune records that in a header byte that was padding, so that consolidation repairs with the build's rule).
 * leann_backend_remove_from_index is the file twin, like leann_backend_add: open -> remove -> consolidate -> save. */
int leann_backend_remove(leann_backend *h, const uint64_t *keys, size_t n, size_t *n_removed);
int leann_backend_consolidate(leann_backend *h);
size_t leann_backend_live_len(const leann_backend *h);
int leann_backend_removed_bitmap(const leann_backend *h, uint8_t *out /* ceil(len/8) */, size_t *n_pending);
int leann_backend_remove_from_index(int backend, const uint64_t *keys, size_t n, size_t dims, const char *index_path_stem);
/* ---- compaction: remove -> consolidate -> compact (csrc/compact.hip, DESIGN.md §5b "Compaction") ----------------------------------
 * A NEW handle holding only the live positions of `h`, renumbered 0 .. live-1 in their old order; `h` is left as it is (close it to
 * give its memory back).  new_to_old (may be NULL): [leann_backend_live_len(h)] OLD global keys, ascending — the caller rewrites its
 * positional id map with it.  key_offset: the new handle's (a shard that moves down after its predecessors shrank);
 * LEANN_KEY_OFFSET_KEEP = that of `h`.
 * Definition.  Let p_0 < p_1 < ... be the live positions of `h`.  The result is the leann_backend_from_arrays[_rows] handle over
 *     rows          row p_j at new position j, byte for byte (the row type is unchanged; the result always owns its rows)
 *     levels        level of p_j at j
 *     level-0 list  of j: the list of p_j, slot for slot, every id mapped through old -> new; 0xFFFFFFFF slots stay where they are
 *     upper lists   the upper lists of p_j in level order, mapped the same way; upper_off = the exclusive prefix sum of the levels
 *     entry         map(entry);  M, M0, max_level and the kind are unchanged
 *     efc, alpha, the Vamana prune form, entry layers and the reference-ef latch are unchanged: with the row type this is every
 *                   piece of state leann_backend_to_rows copies, so a later remove + consolidate on the result repairs by the build's rule
 *     removal state none: nothing removed, no live mask, live_len == len; leann_backend_save writes an ordinary file and deletes a
 *                   stale sidecar.  (leann_backend_add on such a file rebuilds over the concatenation: its levels are no longer the
 *                   builder's hash of the position.)
 * Rows large enough for the row screen get their planes cut by the rule of leann_backend_build_device.  Nothing is searched, pruned
 * or rounded: a walk of the result returns, through the map, the keys, f32 distance bits, counts and counters of the same walk of `h`
 * (the map is monotone, so ties broken by the lower key stay).
 * Checked before any device work, each message naming the way out:  live lists still name removed positions (n_pending > 0), or the
 * entry point is removed -> LEANN_ERR_INVALID (call leann_backend_consolidate first);  nothing live -> LEANN_ERR_INVALID;  NULL `h` /
 * `out` -> LEANN_ERR_INVALID;  a composite handle -> LEANN_ERR_UNSUPPORTED (compact each leann_backend_shard with key_offset = the
 * running sum of the live lengths, then leann_sharded_from_handles);  a recompute-on handle -> LEANN_ERR_UNSUPPORTED (it cannot
 * consolidate, so its lists keep naming removed positions).  A live list that names a removed id although n_pending == 0 is found on
 * the device -> LEANN_ERR_INVALID ("inconsistent graph"), no handle made.
 * Allowed: f32 handles with owned or borrowed rows; bf16 handles with n_pending == 0 (e.g. f32 -> remove -> consolidate ->
 * leann_backend_to_rows, which carries the removals over); a handle without removals (a plain copy, identity map).
 * Not concurrent with searches on `h`, like remove and consolidate.  Peak device memory is `h` plus the result; compacting in place
 * is out of scope. */
#define LEANN_KEY_OFFSET_KEEP UINT64_MAX
int leann_backend_compact(const leann_backend *h, uint64_t key_offset, leann_backend **out, uint64_t *new_to_old);
/* file twin, like leann_backend_remove_from_index: open -> consolidate if lists still name removed positions -> compact -> save.
 * new_to_old (may be NULL) holds `cap` entries; *n_live (may be NULL) = the live positions, set whenever the file opens.
 * cap < live positions -> LEANN_ERR_INVALID naming the size needed, nothing written.  Nothing removed: identity map, file untouched. */
int leann_backend_compact_index(int backend, size_t dims, const char *index_path_stem,
                                uint64_t *new_to_old, size_t cap, size_t *n_live);
/* ---- appending to a handle (csrc/build.hip, DESIGN.md §5 "Append to a handle") -----------------------------------------------------
 * A NEW handle that continues the build of `h` with n more rows; `h` is only read and left as it is (close it to give its memory
 * back).  leann_backend_append takes host rows [n x dims]; leann_backend_append_device rows on h's device, [n x ld] with ld >= dims
 * and ld % 4 == 0.  leann_backend_add is the file twin (HNSW only, and it rebuilds an index whose levels are not the builder's hash).
 * Definition.  Let n_old = leann_backend_len(h).  The result is a handle over n_old + n positions, on h's device, with h's key
 * offset: the key of new row i is key_offset + n_old + i.
 *     rows          [0, n_old): h's rows, byte for byte (also when h borrowed them); then the new rows at h's pitch, zero padded.  The
 *                   result always owns its rows.
 *     levels        positions < n_old keep the level they have in h, whatever made it (the builder, leann_backend_from_arrays, a
 *                   compaction); positions >= n_old get the builder's hash of the position.  upper_off = the exclusive prefix sum of
 *                   that table, which needs h's upper_off to be the prefix sum of h's levels: so for every built, opened or compacted
 *                   handle; a leann_backend_from_arrays handle where it is not -> LEANN_ERR_INVALID naming upper_off.  There is no
 *                   rebuild path: an append always continues.
 *     graph         what the builder makes when it continues from h's lists: the stored link distances recomputed from the rows, the
 *                   pending area empty, the new positions inserted in the builder's hash order among themselves, in batches of at
 *                   most 1 / LEANN_BUILD_BATCH_FRACTION (default 1/8) of the positions linked so far.  HNSW starts from h's entry and
 *                   max_level, which move to a new row that hashes to a higher level.  Vamana keeps h's medoid as the entry (not
 *                   recomputed), uses h's alpha and prunes by the form h RECORDED (one- or two-stage), whatever
 *                   LEANN_VAMANA_TWO_STAGE says now; LEANN_VAMANA_PENDING is read as for a build, there are no refine passes, and
 *                   the final flush runs over all positions.
 *     carried over  efc, alpha, the kind, M, M0, the Vamana prune form, the reference-ef latch and h's coalescing configuration (or
 *                   the default): the state leann_backend_to_rows copies.
 *     removals      carried over: the bitmap extended with zero bits, the live mask uploaded, n_pending counted again on the device
 *                   (lists of new rows may name removed positions that walks still route through, as after leann_backend_add);
 *                   live_len = h's + n.  A later remove, consolidate or compact on the result behaves as on any handle.
 * Rows large enough for the row screen get their planes cut by the rule of leann_backend_build_device.  A leann_filter registered on
 * `h` stays valid for `h` only: on the result it is refused with LEANN_ERR_INVALID ("filter belongs to another handle").  n == 0
 * gives a plain copy.
 * Checked before any device work, each message naming the way out:  NULL `h` / `out`, n > 0 rows with a NULL pointer, ld < dims,
 * ld % 4 != 0, n_old + n >= 2^31 -> LEANN_ERR_INVALID;  a bf16 handle -> LEANN_ERR_UNSUPPORTED (the builder reads f32 rows: rebuild with
 * leann_backend_build_rows);  a recompute-on handle -> LEANN_ERR_UNSUPPORTED (leann_recompute_build_index);  a composite handle ->
 * LEANN_ERR_UNSUPPORTED (append to the last leann_backend_shard, then leann_sharded_from_handles);  a Vamana handle built with
 * LEANN_VAMANA_NAV=1 -> LEANN_ERR_UNSUPPORTED (an experiment knob: rebuild).  On any error *out is NULL, nothing of the call's stays
 * allocated and `h` answers as before.
 * Not concurrent with remove, consolidate or searches on `h`, like compact.  Peak device memory is `h` plus the result plus the
 * builder's scratch; appending in place is out of scope. */
int leann_backend_append(const leann_backend *h, const float *vectors, size_t n, leann_backend **out);
int leann_backend_append_device(const leann_backend *h, const float *d_vectors, size_t n, size_t ld, leann_backend **out);
/* the sidecar's writer and validator on their own (no handle, no device): `bitmap` / `bitmap_out` hold ceil(n/8) bytes */
int leann_tombstones_write(const char *path, const uint8_t *bitmap, uint64_t n, uint64_t n_pending);
int leann_tombstones_read(const char *path, uint64_t n_expected, uint8_t *bitmap_out, uint64_t *n_removed, uint64_t *n_pending);

/* ---- roofline accounting -------------------------------------------------------
 * Totals accumulated over every search call on the handle since the last reset. */
typedef struct {
    uint64_t n_queries;
    uint64_t n_dist_evals;   /* base vectors whose distance was computed (distinct per level) */
    uint64_t n_hops_base;    /* expansions on level 0 */
    uint64_t n_hops_upper;   /* expansions on levels >= 1 */
    uint64_t n_table_overflow; /* queries re-run with the global-memory visited table */
    uint64_t algorithmic_bytes; /* n_dist_evals*dims*4 + n_hops_base*M0*4 + n_hops_upper*M*4 */
} leann_search_stats;
int leann_backend_stats(const leann_backend *h, leann_search_stats *out, int reset);

/* =================================================================================================
 * Device-resident additive API (no reference counterpart): the same operations with operands that
 * already live in HBM, on a caller-supplied HIP stream (void* = hipStream_t, NULL = default).
 * Used by bench.py, the sharded searcher and the recompute path.
 * ============================================================================================== */

/* In-memory index straight from device-resident rows (no file round trip).
 * d_vectors: [n x ld] f32 in HBM, ld % 4 == 0, ld >= dims, padding zero; borrowed if `take_copy`
 * is 0 (must outlive the handle).  key_offset is added to every returned key (shard rebasing,
 * SURVEY.md §8e).  graph_degree: HNSW [2, 64], DiskANN [2, 128], as leann_backend_build. */
int leann_backend_build_device(int backend, const float *d_vectors, size_t n, size_t dims,
                               size_t ld, size_t graph_degree, size_t complexity, int device,
                               uint64_t key_offset, int take_copy, leann_backend **out);
/* Wrap host-side flat graph arrays + host rows into a device index.  M, M0 in [1, 128]. */
int leann_backend_from_arrays(int backend, const float *vectors, size_t n, size_t dims,
                              uint32_t M, uint32_t M0, uint32_t max_level, uint32_t entry,
                              const uint8_t *levels, const uint32_t *upper_off,
                              const uint32_t *adj0, const uint32_t *adjU, size_t n_upper_lists,
                              int device, uint64_t key_offset, leann_backend **out);
/* Copy the graph back to host arrays (sizes from leann_backend_graph_info). */
int leann_backend_graph_info(const leann_backend *h, uint64_t *info /* n,dims,ld,M,M0,max_level,entry,n_upper_lists */);
int leann_backend_graph_export(const leann_backend *h, uint8_t *levels, uint32_t *upper_off,
                               uint32_t *adj0, uint32_t *adjU, float *vectors /* [n x dims] or NULL */);
/* Persist an in-memory index: "<stem>.index" / ".diskann" */
int leann_backend_save(const leann_backend *h, const char *index_path_stem);

/* d_stats: optional [nq x 4] u32: distance evaluations, level-0 hops, upper-level hops, visited-set level (0 = the LDS
 * table sufficed, 1 / 2 = the query moved to a pooled table in HBM, 3 = even the last level filled up: that query's count is 0
 * and the host-pointer entry points return LEANN_ERR_OVERFLOW; the pools are sized so that 3 cannot occur). */
int leann_backend_search_batch_device(const leann_backend *h, const float *d_queries, size_t nq,
                                      size_t top_k, size_t complexity, uint64_t *d_keys,
                                      float *d_dists, uint32_t *d_counts, uint32_t *d_stats,
                                      void *stream);
/* ... with a device-resident allow-bitmap (see leann_backend_search_filtered) */
int leann_backend_search_filtered_batch_device(const leann_backend *h, const float *d_queries,
                                               size_t nq, size_t top_k, size_t complexity,
                                               const uint8_t *d_allow, size_t allow_stride,
                                               uint64_t *d_keys, float *d_dists, uint32_t *d_counts,
                                               uint32_t *d_stats, void *stream);
int leann_backend_search_filtered_exact_batch_device(const leann_backend *h, const float *d_queries,
                                                     size_t nq, size_t top_k, const uint8_t *d_allow,
                                                     size_t allow_stride, uint64_t *d_keys, float *d_dists,
                                                     uint32_t *d_counts, void *stream);
/* device pointer of the rows (for ground-truth scans); NULL for a composite handle and for a handle without f32 rows (bf16 or int8 rows) */
const float *leann_backend_device_rows(const leann_backend *h);

/* ---- row types (additive; DESIGN.md "bf16 rows", "int8 rows") ----------------------------------------------------------------------------------
 * The rows of a stored-vector index are f32 (the default everywhere, and exactly the code paths of before) or bf16, chosen when the
 * index is made.  With r(x) = f32 -> bf16, round to nearest even (a NaN stays a NaN), and w(b) = b << 16 the exact widening:
 *     a bf16 index over rows X IS the f32 index over w(r(X)) with the same graph —
 * every search returns, bit for bit (keys, f32 distance bits, counts, the four per-query stats), what the f32 kernels return on a
 * leann_backend_from_arrays handle made from the same graph arrays and the rows w(r(X)).  Half the device memory, half the index file
 * (LEANNGX1 version 3: the header and graph arrays of version 1, then bf16 rows [n x dims]; leann_backend_open detects it), half
 * the row traffic per evaluation (leann_search_stats.algorithmic_bytes counts dims * 2).
 * On a bf16 handle: leann_backend_graph_export with vectors != NULL writes w(rows); leann_backend_device_rows returns NULL; removal
 * (leann_backend_remove, live_len, removed_bitmap, the tombstone sidecar) works; filter mode 2 picks the walk.
 * LEANN_ERR_UNSUPPORTED with a message naming the way out: exact filtered search and filter mode 1 (use the walk), leann_backend_
 * consolidate (removals stay tombstones), leann_backend_add, leann_backend_append and leann_backend_remove_from_index (rebuild; or remove + save),
 * leann_backend_set_row_screen (no f32 planes exist), leann_backend_open with a device list on a version-3 file (build the shards
 * and use leann_sharded_from_handles: bf16 shards work, mixing row types -> LEANN_ERR_INVALID).
 *
 * int8 rows (LEANN_ROWS_I8): one power-of-two scale per COLUMN and 8-bit codes.  For rows X [n x dims], all finite:
 *     amax_j = max_i |x_ij|;   e_j = the largest integer in [-32, 32] with amax_j * 2^e_j <= 127 (0 when amax_j == 0);
 *     c_ij = clamp(rne(x_ij * 2^e_j), -127, 127)   (the product taken in f32, rne = round to nearest, ties to even; -128 never occurs);
 *     Xq_ij = (float)c_ij * 2^-e_j                  (exact);
 *     an int8 index over rows X IS the f32 index over Xq with the same graph —
 * bit for bit as above (keys, distance bits, counts, the four stats; algorithmic_bytes counts dims * 1).  A quarter of the device
 * memory and of the row traffic; LEANNGX1 version 4: the header and graph arrays of version 1, then int8 exps [dims], then the codes
 * [n x dims] in element order (validated on open: file length, |e_j| <= 32, no code -128, every id and offset against n).
 * A non-finite element -> LEANN_ERR_INVALID naming the row and column, before any graph work.  The kernels apply the scales to the
 * query (q_j * 2^-e_j, exact); a query element with 0 < |q_j| < 2^-90 may underflow there and is out of scope.
 * On an int8 handle everything said of a bf16 handle above holds with "int8" for "bf16" and version 4 for version 3: what works
 * (every search entry point that walks, filter modes 0 and 2, removal and its sidecar, save / open, leann_backend_compact with
 * nothing pending — codes byte for byte, exponents carried —, leann_sharded_from_handles over int8 shards, each with its own
 * exponents) and what is refused with LEANN_ERR_UNSUPPORTED (exact filtered search and mode 1, consolidate, add, append,
 * remove_from_index, set_row_screen, open of a version-4 file with a device list, leann_backend_to_rows from int8 or bf16 -> int8).
 * Measured at 10M x 768 (profiles/i8_rows.md): 1.09 x the bf16 index's queries/s, recall@10 0.0104 below the f32 index's at the same
 * complexity and regained with a beam of 68 for 56; other widths, filtered, wide-list and small-batch throughput: not measured.
 * An unknown row_type -> LEANN_ERR_INVALID before any device work. */
enum { LEANN_ROWS_F32 = 0, LEANN_ROWS_BF16 = 1, LEANN_ROWS_FEATURES = 2 /* recompute-on: no vectors */,
       LEANN_ROWS_I8 = 4 /* 3 stays unassigned: it has always been refused as an unknown row type, and callers may rely on that */ };
/* the handle's row type (a composite handle: its shards' common type); -1 for NULL */
int leann_backend_row_type(const leann_backend *h);
/* host helper, no device: out[i] = r(in[i]) */
int leann_round_bf16(const float *in, size_t n, uint16_t *out);
/* host helper, no device: the int8 definition above on rows in [n x d] -> exps [d], codes [n x d]: the reference quantiser the device
 * kernels are held to.  A non-finite element -> LEANN_ERR_INVALID naming the first one in row-major order. */
int leann_quantize_i8(const float *in, size_t n, size_t d, int8_t *exps, int8_t *codes);
/* leann_backend_build / _build_device / _from_arrays with a row type; LEANN_ROWS_F32 is the existing call, bit for bit.
 * LEANN_ROWS_BF16 (LEANN_ROWS_I8): the rows are rounded (quantised) first and the graph is built by the same builder on w(r(X))
 * (on Xq), so the index is reproducible from its file alone; what follows holds for int8 with Xq for w(r(X)).  build_device_rows: may_overwrite != 0 lets the library overwrite d_vectors with w(r(X)) and build on them
 * in place; 0 takes a transient f32 copy, freed after the build, and the caller's rows come back untouched.  Either way the handle
 * owns its bf16 rows and keeps no f32 rows (d_vectors need not outlive the call); peak device memory is f32 + bf16 rows
 * (the f32 rows being the caller's with may_overwrite, else the library's transient copy beside them; the build cuts no row-screen
 * planes for rows it is about to drop).  The host-pointer build uploads its own copy and builds in place. */
int leann_backend_build_rows(int backend, const float *vectors, size_t n, size_t dims, size_t graph_degree,
                             size_t complexity, int row_type, const char *index_path_stem);
int leann_backend_build_device_rows(int backend, float *d_vectors, size_t n, size_t dims, size_t ld, size_t graph_degree,
                                    size_t complexity, int device, uint64_t key_offset, int row_type, int may_overwrite,
                                    leann_backend **out);
int leann_backend_from_arrays_rows(int backend, const float *vectors, size_t n, size_t dims,
                                   uint32_t M, uint32_t M0, uint32_t max_level, uint32_t entry,
                                   const uint8_t *levels, const uint32_t *upper_off,
                                   const uint32_t *adj0, const uint32_t *adjU, size_t n_upper_lists,
                                   int device, uint64_t key_offset, int row_type, leann_backend **out);
/* A new handle with the SAME graph (copied) and the rows of `h` in another type: today F32 -> BF16 and F32 -> I8 only — the migration path of an
 * existing f32 index (the graph stays the one built on the exact rows; the definition above holds for the result).  `h` is left as
 * it is.  LEANN_ERR_UNSUPPORTED for a composite handle (convert the shards, then leann_sharded_from_handles), a recompute-on handle
 * and from a bf16 or int8 handle to anything.  Removals of `h` are carried over. */
int leann_backend_to_rows(const leann_backend *h, int row_type, leann_backend **out);
/* the rows of a bf16 handle as stored, in element order; LEANN_ERR_UNSUPPORTED for any other handle */
int leann_backend_rows_export_bf16(const leann_backend *h, uint16_t *out /* [n x dims] */);
/* the column exponents and the codes of an int8 handle as stored, in element order; LEANN_ERR_UNSUPPORTED for any other handle */
int leann_backend_rows_export_i8(const leann_backend *h, int8_t *exps /* [dims] */, int8_t *rows /* [n x dims] */);

/* Deterministic synthetic rows written straight into HBM; bit-identical to
 * oracle/oracle.c:orc_gen_rows. */
int leann_synth_rows_device(uint64_t seed, uint32_t dims, uint32_t ld, uint32_t r,
                            uint32_t n_clusters, float sigma, uint32_t stream_id, uint64_t i0,
                            uint64_t n, float *d_out, void *stream);

/* Exact inner-product top-k of every query against all rows — the arithmetic of
 * RecomputeSearcher::search, src/index/recompute.rs:96-109 (scores = raw dot, descending,
 * ties -> lower position), with the embeddings already materialised in HBM.
 * allow_mask: optional N-bit device bitmap (early filter, recompute.rs:66-71). */
int leann_scan_topk_device(const float *d_rows, size_t n, size_t dims, size_t ld,
                           const float *d_queries, size_t nq, size_t top_k,
                           const uint8_t *d_allow_mask, uint64_t key_offset, uint64_t *d_keys,
                           float *d_scores, uint32_t *d_counts, void *stream);

/* ---- recompute search ("pruned" index, no stored vectors) -----------------------------------------
 * RecomputeSearcher::search(query_embedding, embedding_provider, top_k, filter)
 * src/index/recompute.rs:52-123 with the provider (src/embedding/mod.rs:112-120; dense + L2-normalise
 * tail of src/embedding/candle.rs:165,218-225) resident on the device:
 *     features [n x h] bf16 (borrowed), weights [h x dims] bf16 (copied, re-tiled),
 *     embedding_i = l2_normalize(W^T f_i)  (bf16 MFMA, f32 accumulate)
 * scores = raw dot product, descending, ties -> lower position; allow_mask = early filter (:66-71).
 * dims in [1, 4096] (the limit of the stored-vector search); dims > 4096 -> LEANN_ERR_INVALID before any device work.  Up to 768
 * columns one workgroup tile holds a whole embedding; wider ones are encoded in column blocks — same arithmetic per
 * column, sums of squares added block after block in a fixed order.  The limit on h depends on the block width: the feature tile
 * [128 x h] and a ring of three slabs one block wide must fit the 160 KiB of LDS, else LEANN_ERR_INVALID.  dims <= 768 keep their one
 * block of ceil(dims / 128) tiles (h <= 496 at dims <= 128, falling to h <= 256 at dims = 641..768, as before); dims > 768 take
 * narrower blocks when the widest does not fit, so h <= 496 at any such width.  Everything built on a handle — the pooled / host / sharded forms,
 * leann_recompute_encode_device, leann_recompute_search_batch*, leann_recompute_build_index — takes the same widths. */
typedef struct leann_recompute leann_recompute;
int leann_recompute_create(const uint16_t *d_features, size_t n, size_t h, const uint16_t *d_weights,
                           size_t dims, int device, uint64_t key_offset, leann_recompute **out);
/* token-level provider: features [n x L x h] bf16 + attention mask [n x L] (0 = padding, NULL = none), L in
 * {1,2,4,8}: embedding_i = l2_normalize(masked_mean_t(W^T f_it)) — mean_pooling of candle.rs:191-216 with
 * count.clamp(1e-9), then l2_normalize :218-225 */
int leann_recompute_create_pooled(const uint16_t *d_features, const uint8_t *d_mask, size_t n,
                                  size_t tokens_per_passage, size_t h, const uint16_t *d_weights,
                                  size_t dims, int device, uint64_t key_offset, leann_recompute **out);
int leann_recompute_search_batch_device(const leann_recompute *r, const float *d_queries, size_t nq,
                                        size_t top_k, const uint8_t *d_allow_mask, uint64_t *d_keys,
                                        float *d_scores, uint32_t *d_counts, void *stream);
/* host-memory twins (SURVEY.md §8b "Recompute boundary"): plain host pointers in, results out; the handle made by
 * create_host owns a device copy of the features.  keys/scores are [nq x top_k] (unused tail: UINT64_MAX / -inf). */
int leann_recompute_create_host(const uint16_t *features, size_t n, size_t h, const uint16_t *weights,
                                size_t dims, int device, uint64_t key_offset, leann_recompute **out);
int leann_recompute_search_batch(const leann_recompute *r, const float *queries, size_t nq, size_t top_k,
                                 const uint8_t *allow_mask, uint64_t *keys, float *scores, uint32_t *counts);
/* Sharded form: `parts` cover consecutive position ranges (part g's key_offset = part g-1's key_offset + its length,
 * a multiple of 8 past the first part's) and may sit on different devices; a search runs every part's fused scan concurrently and
 * merges the per-part lists by (score descending, key ascending) — bit for bit the answer of one handle over all passages.  The
 * queries, the allow mask (over ALL positions, first part's first position = bit 0) and the results live on the first part's
 * device.  The parts are borrowed: close the composite handle first.  encode / build_index apply to the parts. */
int leann_recompute_create_sharded(const leann_recompute *const *parts, size_t n_parts, leann_recompute **out);
/* materialise embeddings of rows [row0, row0+rows) into d_out [rows x ceil4(dims)] (validation) */
int leann_recompute_encode_device(const leann_recompute *r, uint64_t row0, uint64_t rows, float *d_out,
                                  void *stream);
size_t leann_recompute_len(const leann_recompute *r);
/* HIP-event milliseconds of the last search call: [0] encode GEMM, [1] scoring GEMM, [2] top-k */
int leann_recompute_last_timing(const leann_recompute *r, float *ms3);
void leann_recompute_close(leann_recompute *r);
/* Recompute-on GRAPH index: HNSW / Vamana whose distances are recomputed from the encoder inputs.  The graph is
 * built on transiently materialised embeddings; the returned searcher keeps the graph, the bf16 features and one
 * f32 per passage (||W^T f||) — no vectors — and evaluates dist = 1 - <f, W q> / ||W^T f|| (== 1 - <e, q>).
 * It is an ordinary leann_backend handle: leann_backend_search* work unchanged (queries in embedding space).
 * graph_degree: HNSW [2, 64], DiskANN [2, 128], as leann_backend_build. */
int leann_recompute_build_index(const leann_recompute *r, int backend, size_t graph_degree, size_t complexity,
                                leann_backend **out);
int leann_backend_feature_rows_export(const leann_backend *h, uint32_t *feat_h, uint32_t *row_bytes, void *out);
/* synthetic encoder inputs (bf16), the recompute twin of leann_synth_rows_device */
/* r_int = 0: h-dimensional cluster+noise features; r_int > 0: intrinsic dimension r_int lifted to width h */
int leann_synth_features_device(uint64_t seed, uint32_t h, uint32_t r_int, uint32_t n_clusters, float sigma,
                                uint32_t stream_id, uint64_t i0, uint64_t n, uint16_t *d_out, void *stream);
int leann_synth_weights_device(uint64_t seed, uint32_t h, uint32_t dims, uint16_t *d_out, void *stream);

/* G-way merge of per-shard top-k lists gathered by RCCL: inputs
 * [n_shards x nq x k_in], ascending (dist, key) per list (descending = 1 for recompute scores);
 * outputs [nq x k_out]. */
int leann_merge_topk_device(const uint64_t *d_keys, const float *d_dists, const uint32_t *d_counts,
                            size_t n_shards, size_t nq, size_t k_in, size_t k_out, int descending,
                            uint64_t *d_out_keys, float *d_out_dists, uint32_t *d_out_counts,
                            void *stream);

/* ---- hybrid rerank for batches (BASELINE configs[4]: DiskANN + hybrid BM25 rerank) ------------------------------------------------
 * The hybrid branch of IndexSearcher::search_with_options (src/index/searcher.rs:146-169) + hybrid_rerank (src/index/bm25.rs:135-170)
 * for nq queries at once, on the lists a leann_backend_search_batch_device call with top_k = fetch_k = 5 * top_k left in HBM:
 * BM25-only hits of bm25_top (the first min(fetch_k, count) positives) are appended with vector score 0.0, both score lists are
 * min-max normalised (the BM25 side over ALL n_docs scores), blended alpha * v + (1 - alpha) * b and stable-sorted descending;
 * the first top_k entries are returned (unused tail: UINT64_MAX / -inf).  Every f32 operation in the reference's order.
 * BM25 scores arrive SPARSE, as the host's Bm25Scorer::search produces them: per query `d_bm25_count[q]` positives (position, score),
 * sorted by score descending, ties by position ascending (Rust's stable sort, bm25.rs:118), rows `bm25_stride` entries apart; every
 * other passage scores 0.0.  compat_polarity != 0: the backend's DISTANCES enter the blend as the reference has it (the
 * worst ANN hit gets the largest vector term); 0: corrected, 1 - dist.  fetch_k <= 256.  Positives beyond `bm25_stride` are dropped
 * (P = min(count, stride): min_b / max_b and the scores then differ from the reference's); leann_bm25_hybrid_rerank_device below is
 * the call without that limit. */
int leann_hybrid_rerank_device(const uint64_t *d_keys, const float *d_dists, const uint32_t *d_counts, size_t nq, size_t fetch_k,
                               const uint32_t *d_bm25_pos, const float *d_bm25_score, const uint32_t *d_bm25_count,
                               size_t bm25_stride, size_t n_docs, float alpha, int compat_polarity, size_t top_k,
                               uint64_t *d_out_keys, float *d_out_scores, uint32_t *d_out_counts, void *stream);

/* ---- BM25 on the device (src/index/bm25.rs:77-122 for batches of queries; DESIGN.md "BM25 on the device") ---------------------------
 * An inverted index in HBM: CSR postings — post_off [n_terms + 1], post_doc (passage positions, strictly ascending within a term's
 * list), post_tf (> 0) — plus the passage lengths; the arrays are host pointers, copied at creation.  A query is its KNOWN tokens in
 * query order (a repeated token appears twice, an unknown one not at all), each with its term id and its idf
 * ln((N - df + 0.5) / (df + 0.5) + 1) computed on the host with libm's logf (bm25.rs:88): the device's logf differs in the last bit.
 * Scores are the reference's f32 arithmetic bit for bit: per passage the contributions idf * (tf * (K1 + 1)) / (tf + K1 * norm) are
 * added in query-token order.  Every argument is validated before any device work (LEANN_ERR_INVALID with a message naming it); the
 * checks of the query arrays are also callable on their own (leann_bm25_check_queries), with no handle and no device.
 * A handle serves one batch at a time (calls on one handle serialise) and holds `leann_bm25_slots` dense accumulators of n_docs
 * floats, sized from a fixed 1 GiB budget (at most 64); a batch is processed in chunks of that many queries.  The *_device calls
 * enqueue on `stream` and return after the stream has finished the batch.  They copy the query tokens and synchronise the stream
 * inside, so the BM25 *_device calls cannot be captured into a HIP graph.  Keys are global positions: the lists of a sharded handle
 * live on the first device of its list, and a BM25 handle created on that device reranks them unchanged. */
typedef struct leann_bm25 leann_bm25;
int leann_bm25_create(size_t n_docs, size_t n_terms, const uint64_t *post_off, const uint32_t *post_doc, const uint32_t *post_tf,
                      const uint32_t *doc_len, float avg_doc_len, int device, leann_bm25 **out);
size_t leann_bm25_len(const leann_bm25 *b);
size_t leann_bm25_slots(const leann_bm25 *b);
void leann_bm25_close(leann_bm25 *b);
/* q_off [nq + 1] from 0, monotone; q_term < n_terms; q_idf finite and >= 0 */
int leann_bm25_check_queries(size_t n_terms, size_t nq, const uint32_t *q_off, const uint32_t *q_term, const float *q_idf);
/* Bm25Scorer::search for nq queries: query i has tokens q_term / q_idf [q_off[i], q_off[i + 1]) in query order (host pointers).
 * pos / scores [nq x top_k]: the positives (> 0.0), score descending, ties by position ascending, unused tail UINT32_MAX / -inf;
 * counts [nq]; optional n_positive [nq] = number of positives, min_max [nq x 2] = min and max over ALL n_docs scores.
 * top_k <= 1024. */
int leann_bm25_search_batch(const leann_bm25 *b, size_t nq, const uint32_t *q_off, const uint32_t *q_term, const float *q_idf,
                            size_t top_k, uint32_t *pos, float *scores, uint32_t *counts, uint32_t *n_positive, float *min_max);
int leann_bm25_search_batch_device(const leann_bm25 *b, size_t nq, const uint32_t *q_off, const uint32_t *q_term, const float *q_idf,
                                   size_t top_k, uint32_t *d_pos, float *d_scores, uint32_t *d_counts, uint32_t *d_n_positive,
                                   float *d_min_max, void *stream);
/* scoring + BM25-only injection + hybrid_rerank (see leann_hybrid_rerank_device) on the lists a search_batch_device call with
 * top_k = fetch_k left in HBM; the BM25 score of a merged key is read from the query's dense score vector, so there is no limit
 * on the number of positives.  fetch_k <= 256, top_k <= 512, alpha in [0, 1]. */
int leann_bm25_hybrid_rerank_device(const leann_bm25 *b, size_t nq, const uint32_t *q_off, const uint32_t *q_term, const float *q_idf,
                                    const uint64_t *d_keys, const float *d_dists, const uint32_t *d_counts, size_t fetch_k,
                                    float alpha, int compat_polarity, size_t top_k,
                                    uint64_t *d_out_keys, float *d_out_scores, uint32_t *d_out_counts, void *stream);
/* The three calls above under an allow-bitmap (DESIGN.md §8c "under a filter"), so that a hybrid query under a metadata filter, or on
 * an index with removed passages, composes with the filtered graph search.  Let A be the positions whose bit is set: bit i & 7 of byte
 * i >> 3 stands for position i, ceil(n_docs / 8) bytes, bits at positions >= n_docs ignored.  Scoring is unchanged — idf, doc_len and
 * avg_doc_len are the corpus's, a filter does not change them — and everything after it sees the score vector restricted to A:
 *   search   the positives at positions in A, score descending, ties by position ascending; n_positive counts the positives in A;
 *            min_max is folded over the scores at positions in A.
 *   hybrid   bm25_top is that search at fetch_k and min_b / max_b are folded over A; the ANN lists enter as given (the caller searched
 *            under the same bitmap) and the BM25 score of a merged key is scores[key], as in the unfiltered call.
 *   empty A  count 0 for that query in both calls, whatever its ANN list holds; n_positive 0; min_max (+inf, -inf), the folds' identities.
 * allow / allow_stride as in leann_backend_search_filtered_batch_device: stride 0 is one bitmap for the batch, otherwise query i uses
 * allow + i * allow_stride, any value >= ceil(n_docs / 8) (no alignment is needed).  allow == NULL with stride 0 is the unfiltered
 * call, bit for bit and launch for launch.  A non-zero stride below ceil(n_docs / 8), or a NULL bitmap with a non-zero stride, is
 * LEANN_ERR_INVALID before any device work, like every other argument.  In the *_device forms the bitmap is in HBM on the handle's
 * device — e.g. what leann_meta_eval_device wrote on the same stream, or leann_backend_filter_bitmap_device — and the host form
 * uploads it.  Like their twins, the *_device calls synchronise the stream inside and cannot be captured into a HIP graph. */
int leann_bm25_search_filtered_batch(const leann_bm25 *b, size_t nq, const uint32_t *q_off, const uint32_t *q_term, const float *q_idf,
                                     size_t top_k, const uint8_t *allow, size_t allow_stride,
                                     uint32_t *pos, float *scores, uint32_t *counts, uint32_t *n_positive, float *min_max);
int leann_bm25_search_filtered_batch_device(const leann_bm25 *b, size_t nq, const uint32_t *q_off, const uint32_t *q_term,
                                            const float *q_idf, size_t top_k, const uint8_t *d_allow, size_t allow_stride,
                                            uint32_t *d_pos, float *d_scores, uint32_t *d_counts, uint32_t *d_n_positive,
                                            float *d_min_max, void *stream);
int leann_bm25_hybrid_rerank_filtered_device(const leann_bm25 *b, size_t nq, const uint32_t *q_off, const uint32_t *q_term,
                                             const float *q_idf, const uint64_t *d_keys, const float *d_dists, const uint32_t *d_counts,
                                             size_t fetch_k, float alpha, int compat_polarity, size_t top_k,
                                             const uint8_t *d_allow, size_t allow_stride,
                                             uint64_t *d_out_keys, float *d_out_scores, uint32_t *d_out_counts, void *stream);

/* ---- metadata filters evaluated on the device (src/index/filter.rs:328-418) ---------------------------------------------
 * A leann_meta is a columnar copy of the passages' metadata in HBM: one column per field (a dotted path, get_nested_value,
 * filter.rs:376-388), per row a tag, a number and a string code.  The caller hands over each row's string (str_blob bytes
 * [str_off[i], str_off[i + 1]) for a STRING row); the library builds the column's dictionary — the distinct strings sorted bytewise
 * ascending, which is Rust's str::cmp order — and the codes.  The dictionary stays on the host, tags / numbers / codes go to the device.
 * `valid`: optional bitmap of the rows whose metadata could be read; an invalid row passes no filter, not even Ne / NotIn / a filter
 * on a missing field.  All arrays are host pointers, copied.  Every argument is validated before any device work (LEANN_ERR_INVALID
 * with a message naming it): a tag above LEANN_META_OTHER, STRING rows without str_off, non-monotone str_off, a duplicate field,
 * n >= 2^32.  A NUMBER row's num is the value's as_f64(); num == NULL with NUMBER rows -> LEANN_ERR_INVALID. */
enum { LEANN_META_MISSING = 0, LEANN_META_NULL = 1, LEANN_META_FALSE = 2, LEANN_META_TRUE = 3, LEANN_META_NUMBER = 4,
       LEANN_META_STRING = 5, LEANN_META_OTHER = 6 /* array / object */ };
typedef struct leann_meta leann_meta;
int leann_meta_create(size_t n, const uint8_t *valid, int device, leann_meta **out);
int leann_meta_add_column(leann_meta *m, const char *field, const uint8_t *tag, const double *num, const char *str_blob,
                          const uint64_t *str_off);
size_t leann_meta_len(const leann_meta *m);
int leann_meta_has_column(const leann_meta *m, const char *field); /* 1 / 0 */
void leann_meta_close(leann_meta *m); /* when no evaluation is in flight */
/* A filter is passed PARSED, as its tree in prefix order: a node, then its n_children subtrees.  The mini-language parser stays above
 * the ABI.  A COND node names a field, one of the twelve FilterOp and a value; a LIST value (In / NotIn) holds `len` scalar values.
 * Limits (csrc/meta_plan.h; LEANN_ERR_INVALID naming the limit): 32 conditions, nesting depth 8, 8 distinct fields, 2^20 32-bit words
 * of number sets and dictionary bitsets per filter; a field without a column is refused by name. */
enum { LEANN_META_COND = 0, LEANN_META_AND = 1, LEANN_META_OR = 2 };
enum { LEANN_META_OP_EQ = 0, LEANN_META_OP_NE, LEANN_META_OP_GT, LEANN_META_OP_GTE, LEANN_META_OP_LT, LEANN_META_OP_LTE, LEANN_META_OP_IN,
       LEANN_META_OP_NOT_IN, LEANN_META_OP_CONTAINS, LEANN_META_OP_STARTS_WITH, LEANN_META_OP_ENDS_WITH, LEANN_META_OP_EXISTS };
enum { LEANN_META_VAL_NULL = 0, LEANN_META_VAL_BOOL = 1, LEANN_META_VAL_NUMBER = 2, LEANN_META_VAL_STRING = 3, LEANN_META_VAL_LIST = 4 };
typedef struct leann_meta_value {
    int32_t type;    /* LEANN_META_VAL_* */
    int32_t boolean; /* BOOL */
    double num;      /* NUMBER */
    const char *str; /* STRING: len bytes, no terminator needed */
    size_t len;      /* STRING: bytes; LIST: elements */
    const struct leann_meta_value *list; /* LIST: elements of the scalar types (a nested list equals nothing) */
} leann_meta_value;
typedef struct leann_meta_node {
    int32_t kind;        /* LEANN_META_COND / AND / OR */
    uint32_t n_children; /* AND / OR */
    const char *field;   /* COND */
    int32_t op;          /* COND: LEANN_META_OP_* */
    leann_meta_value value; /* COND */
} leann_meta_node;
/* MetadataFilter::matches for every row at once: bit i of bitmap = row i is valid and matches.  bitmap: host, ceil(n / 8) bytes, pad
 * bits zero; n_allowed: optional.  One kernel (meta_eval_kernel) reads only the columns the filter names. */
int leann_meta_eval(const leann_meta *m, const leann_meta_node *nodes, size_t n_nodes, uint8_t *bitmap, size_t *n_allowed);
/* The same into device memory on the store's device: d_bitmap [ceil(n / 8)] = valid AND match AND d_and (optional device bitmap);
 * no byte behind ceil(n / 8) is written.  d_n_allowed: optional device counter, set to the number of allowed rows.  The filter is
 * compiled on the host, the work is enqueued on `stream` and the call returns without waiting for it.  A filter that needs number
 * sets or dictionary bitsets (In / NotIn lists, Contains, EndsWith) copies them to the device from pageable host memory with a
 * stream-ordered copy, so leann_meta_eval_device cannot be captured into a HIP graph; calls on one store and one stream reuse one
 * scratch block, calls on different streams do not disturb each other.  The bitmap is an ordinary allow-bitmap: it feeds
 * leann_backend_search_filtered[_exact]_batch_device, leann_scan_topk_device and leann_recompute_search_batch_device. */
int leann_meta_eval_device(const leann_meta *m, const leann_meta_node *nodes, size_t n_nodes, const uint8_t *d_and, uint8_t *d_bitmap,
                           uint32_t *d_n_allowed, void *stream);
/* n_out filters -> n_out bitmaps in one pass over the columns; bitmap i = what leann_meta_eval[_device] writes for filter i, bit for
 * bit.  Filter i is nodes[node_off[i] .. node_off[i + 1]) in prefix order (node_off[0] == 0, monotone).  Bitmap i starts at
 * bitmaps + i * stride: any stride >= ceil(n / 8) and any base alignment; of a row only the first ceil(n / 8) bytes are written (pad
 * bits zero), the bytes between rows are left as they are.  Equal filters (the same compiled program, csrc/meta_batch_plan.h) are
 * evaluated once: *n_distinct (optional) says how many programs ran.  A launch of meta_eval_batch_kernel takes up to 64 distinct
 * programs over up to 16 distinct columns and 2^20 words of sets / bitsets; a batch beyond that is cut into several launches, never
 * refused.  n_allowed [n_out]: optional counts.  n_out == 0 is LEANN_OK with nothing written.
 * The _device form compiles and plans on the host, copies programs, pairs and words into a per-stream scratch block of the store
 * with ONE stream-ordered copy from pageable host memory (so, like its single twin, it cannot be captured into a HIP graph), enqueues
 * one kernel per launch on `stream` and returns without waiting.  d_and: optional, ONE device bitmap ANDed into every output.
 * d_n_allowed [n_out]: optional device counters, zeroed on the stream and then set.  Every argument is validated before any device
 * work, LEANN_ERR_INVALID naming it: a null store, nodes, offsets or bitmaps; node_off[0] != 0 or non-monotone offsets; stride <
 * ceil(n / 8); a filter meta_compile refuses, as "filter <i>: <its message>". */
int leann_meta_eval_batch(const leann_meta *m, const leann_meta_node *nodes, const size_t *node_off, size_t n_out,
                          uint8_t *bitmaps, size_t stride, size_t *n_allowed /* [n_out], optional */, size_t *n_distinct /* optional */);
int leann_meta_eval_batch_device(const leann_meta *m, const leann_meta_node *nodes, const size_t *node_off, size_t n_out,
                                 const uint8_t *d_and /* optional, ONE bitmap for all */, uint8_t *d_bitmaps, size_t stride,
                                 uint32_t *d_n_allowed /* [n_out], optional */, size_t *n_distinct /* optional */, void *stream);
/* nq queries, query i under filter i: evaluate, then search.  Defined by delegation: query i's keys, f32 distance bits, count and
 * four stats are what leann_backend_search_filtered_batch_device (mode 0, the walk) or leann_backend_search_filtered_exact_batch_device
 * (mode 1; d_stats is not written) return for bitmap i = filter i evaluated by leann_meta_eval_device — on a composite, narrow-row or
 * recompute-on handle too, their refusals (LEANN_ERR_UNSUPPORTED for mode 1 on narrow rows and recompute-on handles) included.  The
 * delegated calls AND the index's live mask themselves.  d_n_allowed [nq]: optional, the rows filter i allows (before the live
 * mask): what a caller needs to split a batch between the modes itself.  The bitmaps live in library scratch, at most 1 GiB at a
 * time: the batch runs in chunks of max(1, 1 GiB / stride) queries, stride = ceil(n / 8) rounded up to 16, each chunk planned,
 * evaluated and searched on its own (LEANN_DEBUG_META_BATCH_BYTES: a test hook that overrides the 1 GiB).  The scratch must outlive
 * the work, so the _device form synchronises `stream` before it returns and cannot be captured into a HIP graph.
 * LEANN_ERR_INVALID before any device work: a null argument or top_k == 0; leann_meta_len(m) != leann_backend_len(h); a store on
 * another device than the handle's (a composite handle: its first device); a mode other than 0 or 1; bad offsets or a bad filter as
 * in leann_meta_eval_batch.  After any error nothing of the call's stays allocated.  The host form takes host pointers for queries
 * and results (stats and n_allowed optional). */
int leann_backend_search_meta_batch_device(const leann_backend *h, const leann_meta *m, const float *d_queries, size_t nq, size_t top_k,
                                           size_t complexity, const leann_meta_node *nodes, const size_t *node_off, int mode /* 0 walk, 1 exact */,
                                           uint64_t *d_keys, float *d_dists, uint32_t *d_counts, uint32_t *d_stats, uint32_t *d_n_allowed, void *stream);
int leann_backend_search_meta_batch(const leann_backend *h, const leann_meta *m, const float *queries, size_t nq, size_t top_k,
                                    size_t complexity, const leann_meta_node *nodes, const size_t *node_off, int mode /* 0 walk, 1 exact */,
                                    uint64_t *keys, float *dists, uint32_t *counts, uint32_t *stats, uint32_t *n_allowed);
/* leann_backend_filter_create with the bitmap evaluated on the device (valid AND match, then the index's live mask) instead of
 * uploaded: the resulting leann_filter is the one leann_backend_filter_create makes from the same bitmap.  leann_meta_len(m) !=
 * leann_backend_len(h) or a store on another device than the handle's (a composite handle: its first device) -> LEANN_ERR_INVALID.
 * A composite handle: evaluated once on the store's device, downloaded, then registered per shard as leann_backend_filter_create does. */
int leann_backend_filter_create_meta(const leann_backend *h, const leann_meta *m, const leann_meta_node *nodes, size_t n_nodes,
                                     leann_filter **out);
/* 0 when LEANN_META_DEVICE=0 is set in the environment (read once, with the other knobs), else 1.  The library's own entry points do
 * not look at it: it is for a host that keeps a per-passage loop beside the device path (host/leann_host.hpp) and wants one switch. */
int leann_meta_device_enabled(void);

/* ---- refining results on exact rows (additive; csrc/refine.hip) -----------------------------------------------------------
 * A bf16 or int8 index walks rounded rows and reports their distances, a recompute-on index 1 - <f, Wq> / ||W^T f||.  Refining is what
 * FAISS IndexRefine and DiskANN's full-precision rerank do: the walk fetches fetch_k >= top_k candidates, only those are scored again
 * on the exact f32 rows, the best top_k are returned.  The exact rows are an object of their own, beside the index: they may sit in
 * HBM or in pinned host memory that the kernel reads in place across the bus (10-40 rows per query), so that an int8 index keeps its
 * quarter of the DEVICE memory.  Every existing entry point, the refusals of narrow-row handles included, is exactly as it was.
 *
 * A leann_exact_rows names f32 rows [n x ld] the device can read, for positions key_offset .. key_offset + n - 1; ld % 4 == 0,
 * ld >= dims, padding zero, dims in [1, 4096], n < 2^32 - 1.
 *   _from_device  borrows rows on `device` (e.g. leann_backend_device_rows of an f32 handle); they must outlive the object.
 *   _from_host    copies host rows [n x dims]: placement LEANN_EXACT_ROWS_HBM into device memory, LEANN_EXACT_ROWS_HOST into a
 *                 library-owned block of pinned, device-mapped host memory (hipHostMalloc; no managed memory, nothing that needs
 *                 XNACK).  If that block cannot be had: LEANN_ERR_DEVICE, the message naming placement 0 as the way out — never a
 *                 silent fall-back.
 *   _open         a "<stem>.embeddings" file (raw LE f32 [n x dims], src/index/embeddings.rs:21-153; `leann build --recompute` writes it
 *                 beside the index) through the reader leann_backend_open uses for a stock directory; a missing file ->
 *                 LEANN_ERR_NOT_FOUND naming `leann build --recompute`, a length that is no whole number of rows -> LEANN_ERR_FORMAT.
 * An unknown placement, dims outside [1, 4096], a null pointer -> LEANN_ERR_INVALID before any device work.  _close waits for the
 * device before it frees what the object owns.
 *
 * leann_rerank_batch_device.  Query q has the candidates d_keys[q * fetch_k + i], i < min(d_counts[q], fetch_k).  A candidate is VALID
 * when key_offset <= key < key_offset + n; every other key — the UINT64_MAX tail value included — is skipped, counted in d_skipped[q]
 * (optional [nq]) and no row is read for it: the kernel range-checks every key before it forms an address, so a list with garbage in
 * it cannot fault the device.  Result: the valid candidates ordered by (dist, key) ascending, the first top_k of them;
 * dist = 1 - canonical dot(q, X[key - key_offset]), the distance the f32 traversal kernels compute (wave_dist_rows, csrc/search.cuh;
 * orc_dist_canon, oracle/oracle.c), so A REFINED DISTANCE IS, BIT FOR BIT, WHAT AN F32 INDEX OVER THE SAME ROWS REPORTS FOR THAT KEY.
 * Unused tail: UINT64_MAX / +inf.  A key listed twice is returned twice.  Limits: 1 <= top_k <= fetch_k <= 1024; the queries have the
 * rows' dims.  Queries, lists and results are on the rows' device.  The call only ENQUEUES one kernel on `stream`: it allocates
 * nothing, copies nothing and does not wait, so it can stand in a captured HIP graph.
 *
 * leann_backend_search_refined_batch_device is defined by delegation: leann_backend_search_filtered_batch_device(h, ..., top_k =
 * fetch_k, complexity, d_allow, allow_stride, ...) into library scratch (d_allow == NULL: the unfiltered search), then the rerank
 * above; d_stats are the walk's.  ef = max(complexity, fetch_k) by the existing rule, so a fetch_k above `complexity` widens the beam.
 * It works on every handle the walk works on — f32, bf16, int8, recompute-on, and composite handles, whose keys are global and whose
 * lists live on the first device.  The scratch must outlive the work, so the call SYNCHRONISES `stream` before it returns and cannot
 * be captured into a HIP graph.  LEANN_ERR_INVALID before any device work, the message naming the argument: a null argument; top_k ==
 * 0, fetch_k > 1024, top_k > fetch_k; the rows' dims differ from the handle's; the rows sit on another device than the handle's (a
 * composite handle: its first); the rows' positions do not cover [key_offset_h, key_offset_h + len) of the handle.  After any error
 * nothing of the call's stays allocated.  leann_backend_search_refined_batch is the host-pointer twin: queries, allow-bitmap(s) and
 * results (stats optional, [nq x 4]) on the host. */
typedef struct leann_exact_rows leann_exact_rows;
enum { LEANN_EXACT_ROWS_HBM = 0, LEANN_EXACT_ROWS_HOST = 1 };
int leann_exact_rows_from_device(const float *d_rows, size_t n, size_t dims, size_t ld, int device, uint64_t key_offset,
                                 leann_exact_rows **out);
int leann_exact_rows_from_host(const float *rows, size_t n, size_t dims, int device, uint64_t key_offset, int placement,
                               leann_exact_rows **out);
int leann_exact_rows_open(const char *embeddings_path, size_t dims, int device, uint64_t key_offset, int placement,
                          leann_exact_rows **out);
size_t leann_exact_rows_len(const leann_exact_rows *r);
int leann_exact_rows_placement(const leann_exact_rows *r); /* -1 for NULL */
void leann_exact_rows_close(leann_exact_rows *r);
int leann_rerank_batch_device(const leann_exact_rows *r, const float *d_queries, size_t nq, const uint64_t *d_keys,
                              const uint32_t *d_counts, size_t fetch_k, size_t top_k, uint64_t *d_out_keys, float *d_out_dists,
                              uint32_t *d_out_counts, uint32_t *d_skipped /* optional [nq] */, void *stream);
int leann_backend_search_refined_batch_device(const leann_backend *h, const leann_exact_rows *r, const float *d_queries, size_t nq,
                                              size_t top_k, size_t fetch_k, size_t complexity, const uint8_t *d_allow,
                                              size_t allow_stride, uint64_t *d_keys, float *d_dists, uint32_t *d_counts,
                                              uint32_t *d_stats, void *stream);
int leann_backend_search_refined_batch(const leann_backend *h, const leann_exact_rows *r, const float *queries, size_t nq,
                                       size_t top_k, size_t fetch_k, size_t complexity, const uint8_t *allow, size_t allow_stride,
                                       uint64_t *keys, float *dists, uint32_t *counts, uint32_t *stats /* optional */);

/* ---- sharded indexes (the reference has no counterpart: IndexSearcher owns one Box<dyn BackendSearcher>,
 * src/index/searcher.rs:68) --------------------------------------------------------------------------------------------------
 * One process, G devices: the composite handle leann_backend_open returns for a device list, or built here from rows / handles.
 * Every leann_backend_search* entry point works on it: the in-traversal allow-bitmap, exact filtered search and registered filters
 * (the bitmap is sliced per shard — interior shard boundaries are multiples of 64 —, every shard answers for its slice, lists are merged
 * by (dist, key): the answer of an unsharded index for exact searches, up to the order of entries with equal distances).  leann_backend_save writes one self-contained file
 * per shard, "<stem>.shard<g>of<G>.index" / ".diskann", which leann_backend_open with a list of G devices loads again; graph export is
 * per shard (leann_backend_shard).  Queries and results of the *_device calls live on the first device of the list.
 * One process per GPU: leann_sharded_attach joins this rank's shard to an RCCL communicator (librccl.so is resolved at run time);
 * a search is the local traversal + ONE ncclAllGather of the packed per-shard block {u64 keys | f32 dists | u32 counts} + the merge
 * kernel on every rank.  All ranks must issue the same calls with the same nq / top_k.
 * In both modes exchange + merge run on the handle's own stream, so the *_async form lets batch i + 1's traversal overlap batch
 * i's exchange (two result slots rotate: wait for ticket t before issuing t + 2). */
typedef struct leann_sharded leann_sharded;
int leann_sharded_open(const char *index_path_stem, int backend, size_t dims, const char *device_spec, leann_sharded **out);
/* the sub-index of shard g of a composite handle as an ordinary handle (borrowed — do not close it; it returns global keys):
 * graph_info / graph_export / feature_rows_export work on it.  leann_backend_shard_count: 0 for a plain handle. */
size_t leann_backend_shard_count(const leann_backend *h);
int leann_backend_shard(const leann_backend *h, size_t g, leann_backend **out);
/* d_vectors[g]: rows of shard g on devices[g] ([rows[g] x ld] f32, borrowed); keys are rebased by the prefix sums of rows[];
 * graph_degree: HNSW [2, 64], DiskANN [2, 128], as leann_backend_build */
int leann_sharded_build_device(int backend, const float *const *d_vectors, const size_t *rows, size_t n_shards, size_t dims,
                               size_t ld, size_t graph_degree, size_t complexity, const int *devices, leann_sharded **out);
/* existing handles (each built with its key_offset); take_ownership: leann_sharded_close closes them */
int leann_sharded_from_handles(leann_backend *const *shards, size_t n_shards, int take_ownership, leann_sharded **out);
/* wrap a one-process group as an ordinary leann_backend handle (closing that handle closes the group) */
int leann_sharded_as_backend(leann_sharded *s, leann_backend **out);
/* RCCL: rank 0 makes the id (128 bytes), the host distributes it by its own means, every rank attaches its shard (collective) */
int leann_rccl_get_unique_id(void *id128);
int leann_sharded_attach(leann_backend *local_shard, const void *unique_id128, int world, int rank, size_t total_rows,
                         leann_sharded **out);
/* d_stats: optional per-query counters [nq x 4], the layout of leann_backend_search_batch_device: one process — evaluations and
 * hops summed over the shards, visited-set level = the highest any shard needed; RCCL — the local shard's */
int leann_sharded_search_batch_device(const leann_sharded *s, const float *d_queries, size_t nq, size_t top_k, size_t complexity,
                                      uint64_t *d_keys, float *d_dists, uint32_t *d_counts, uint32_t *d_stats, void *stream);
int leann_sharded_search_batch_device_async(const leann_sharded *s, const float *d_queries, size_t nq, size_t top_k,
                                            size_t complexity, uint64_t *d_keys, float *d_dists, uint32_t *d_counts,
                                            uint32_t *d_stats, void *stream, uint64_t *ticket);
int leann_sharded_wait(const leann_sharded *s, uint64_t ticket, void *stream); /* `stream` waits for that exchange + merge */
size_t leann_sharded_len(const leann_sharded *s);    /* rows over all shards */
size_t leann_sharded_shards(const leann_sharded *s);
void leann_sharded_close(leann_sharded *s);

/* Environment knobs (LEANN_COALESCE, LEANN_HNSW_REFERENCE_EF, the LEANN_DEBUG_* test hooks) are read ONCE, when the library is first
 * used — no search call touches the environment.  A test that changes one of them afterwards calls this to have it read again. */
void leann_debug_reload_env(void);
/* Test hook: how many device blocks the library owns at this moment — everything its handles, filters and calls in flight hold,
 * but neither leann_device_malloc memory (the caller's) nor blocks resting in the library's scratch pool.  Back at its earlier
 * value once whatever was made since has been closed. */
uint64_t leann_debug_device_blocks(void);

/* raw device memory helpers so that non-torch hosts (the C++ CLI, ctypes tests) need no HIP binding */
int leann_device_count(int *n);
int leann_device_malloc(int device, size_t bytes, void **out);
int leann_device_free(void *p);
int leann_device_upload(void *d_dst, const void *h_src, size_t bytes);
int leann_device_download(void *h_dst, const void *d_src, size_t bytes);
int leann_device_sync(int device);

#ifdef __cplusplus
}
#endif
#endif
