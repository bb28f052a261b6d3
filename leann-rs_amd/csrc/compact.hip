// compact.hip — remove -> consolidate -> COMPACT (DESIGN.md §5b "Compaction"; the definition: include/leann_backend.h).
//
// After a consolidate the removed positions are unreachable and no live list names them, so dropping them is a pure renaming: the
// live positions p_0 < p_1 < ... become 0 .. live - 1 in their old order, rows and lists move with them, every id in a list goes
// through old -> new.  Nothing is searched, pruned or rounded, and no row and no list crosses to the host:
//
//   position map   old_to_new u32 [n] (LEANN_EMPTY for removed positions) and new_to_old u32 [live], written on the host from the
//                  handle's removal bitmap (n / 8 bytes in, 8 n bytes out — not the hot part) and uploaded;
//   rows           gather_rows_kernel: row_bytes-pitched rows by new_to_old in 16-byte pieces.  One kernel for both row types: an f32
//                  pitch is ld * 4 with ld % 4 == 0, a bf16 or int8 pitch is a multiple of 128 B in its own element order, which a byte copy keeps;
//   levels         gather_levels_kernel; upper_off = their exclusive prefix sum, on the host as the builder's alloc_graph_arrays does;
//   lists          remap_lists_kernel, once for level 0 and once for the upper array: the lists of a node are one contiguous run of
//                  slots in either array (level 0: one list at the node's position; upper: `level` lists from upper_off), so both
//                  are "copy the run of p_j to the run of j, ids mapped".  A live list that names a removed id cannot occur once
//                  n_pending == 0; it is checked anyway (a device flag set by an ordinary atomic) and refused as an inconsistent graph.
//
// Peak device memory is the source handle plus the result (an in-place form is out of scope).  Like remove and consolidate, compaction
// is not concurrent with searches on the source handle.
#include "common.cuh"
#include "internal.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <sys/stat.h>
#include <vector>

// A tile = `tile_rows` consecutive NEW rows = tile_rows * pieces 16-byte pieces, contiguous in dst; piece t of a tile comes from
// row new_to_old[row0 + t / pieces].  Each thread has up to four loads in flight before its first store.
#define GATHER_THREADS 256
#define GATHER_UNROLL 4
__global__ void __launch_bounds__(GATHER_THREADS) gather_rows_kernel(const uint4 *__restrict__ src, uint4 *__restrict__ dst,
                                                                     const uint32_t *__restrict__ new_to_old, uint64_t live,
                                                                     uint32_t pieces /* 16-byte pieces per row */, uint32_t tile_rows) {
    const uint64_t tiles = (live + tile_rows - 1) / tile_rows;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t row0 = tile * tile_rows;
        const uint32_t rows = live - row0 < tile_rows ? (uint32_t)(live - row0) : tile_rows, items = rows * pieces;
        uint4 *out = dst + row0 * pieces;
        for (uint32_t base = threadIdx.x; base < items; base += GATHER_THREADS * GATHER_UNROLL) {
            uint4 v[GATHER_UNROLL];
#pragma unroll
            for (int u = 0; u < GATHER_UNROLL; u++) {
                const uint32_t t = min(base + u * GATHER_THREADS, items - 1); // (past the tile: its last piece again, not stored)
                const uint32_t r = t / pieces;
                v[u] = src[(uint64_t)new_to_old[row0 + r] * pieces + (t - r * pieces)];
            }
#pragma unroll
            for (int u = 0; u < GATHER_UNROLL; u++) {
                const uint32_t t = base + u * GATHER_THREADS;
                if (t < items) out[t] = v[u];
            }
        }
    }
}

__global__ void gather_levels_kernel(const uint8_t *__restrict__ levels, const uint32_t *__restrict__ new_to_old, uint32_t live,
                                     uint8_t *__restrict__ out) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < live) out[j] = levels[new_to_old[j]];
}

// One wave per new node j: its run of `cnt` lists of W slots moves from list `src_first` to list `dst_first`, ids mapped.
// levels == null: level 0 (cnt = 1, the lists sit at the positions); else the upper array (cnt = the node's level, from upper_off).
// src_lists: how many lists src holds.  *bad is set when a slot names a removed or unknown position, or a run leaves src.
__global__ void __launch_bounds__(256) remap_lists_kernel(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, uint32_t W,
                                                          const uint32_t *__restrict__ new_to_old, const uint32_t *__restrict__ old_to_new,
                                                          uint32_t n_old, uint32_t live, const uint8_t *__restrict__ new_levels,
                                                          const uint32_t *__restrict__ src_upper_off, const uint32_t *__restrict__ dst_upper_off,
                                                          uint64_t src_lists, uint32_t *__restrict__ bad) {
    const uint32_t lane = threadIdx.x & 63u, waves = (gridDim.x * blockDim.x) >> 6;
    bool inconsistent = false;
    for (uint32_t j = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; j < live; j += waves) {
        const uint32_t p = new_to_old[j];
        const uint32_t cnt = new_levels ? new_levels[j] : 1u;
        if (cnt == 0) continue;
        const uint32_t first = new_levels ? src_upper_off[p] : p;
        if ((uint64_t)first + cnt > src_lists) { inconsistent = true; continue; } // the run would leave the source array
        const uint32_t *in = src + (size_t)first * W;
        uint32_t *out = dst + (size_t)(new_levels ? dst_upper_off[j] : j) * W;
        for (uint32_t s = lane; s < cnt * W; s += 64) {
            uint32_t id = in[s];
            if (id != LEANN_EMPTY) {
                id = id < n_old ? old_to_new[id] : LEANN_EMPTY;
                inconsistent |= id == LEANN_EMPTY; // names a removed (or unknown) position
            }
            out[s] = id;
        }
    }
    if (inconsistent) atomicOr(bad, 1u);
}

namespace {
// device events around the phases, made only when LEANN_LOG=info asks for the timing line (scripts/compact_bench.py reads it)
struct PhaseClock {
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    bool on = false;
    PhaseClock() {
        if (!leann_log_enabled(LEANN_LOG_INFO)) return;
        on = true;
        for (hipEvent_t &e : ev)
            if (hipEventCreate(&e) != hipSuccess) { e = nullptr; on = false; (void)hipGetLastError(); }
    }
    ~PhaseClock() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    void mark(int i) { if (on) (void)hipEventRecord(ev[i], nullptr); }
    float ms(int a, int b) {
        float t = 0.f;
        return on && hipEventElapsedTime(&t, ev[a], ev[b]) == hipSuccess ? t : 0.f;
    }
};

struct CompactChecked { // what the precondition checks hand on
    size_t n = 0, live = 0;
    std::vector<uint8_t> removed; // snapshot of the source's bitmap (empty: nothing removed)
};

int check_source(const leann_backend *hc, CompactChecked *c) {
    if (hc->sharded) {
        leann_set_error("leann_backend_compact: not available on a composite handle; compact each shard (leann_backend_shard) with key_offset = "
                        "the running sum of the live lengths, then leann_sharded_from_handles");
        return LEANN_ERR_UNSUPPORTED;
    }
    if (hc->g.feat_h) {
        leann_set_error("leann_backend_compact: a recompute-on index cannot consolidate, so its lists keep naming removed positions; "
                        "rebuild it from the live rows");
        return LEANN_ERR_UNSUPPORTED;
    }
    leann_backend *src = const_cast<leann_backend *>(hc);
    std::lock_guard<std::mutex> lk(src->mu); // (leann_backend_remove changes the bitmap)
    c->n = hc->g.n;
    c->live = c->n - hc->n_removed;
    if (hc->n_pending) {
        leann_set_error("leann_backend_compact: live lists still name %zu removed positions; call leann_backend_consolidate first", hc->n_pending);
        return LEANN_ERR_INVALID;
    }
    if (c->live == 0) {
        leann_set_error("leann_backend_compact: nothing is live (%zu of %zu positions removed)", hc->n_removed, c->n);
        return LEANN_ERR_INVALID;
    }
    if (hc->n_removed) c->removed = hc->removed;
    const uint32_t e = hc->g.entry;
    if (!c->removed.empty() && ((c->removed[e >> 3] >> (e & 7)) & 1)) {
        leann_set_error("leann_backend_compact: the entry point is removed; call leann_backend_consolidate first (it replaces it)");
        return LEANN_ERR_INVALID;
    }
    return LEANN_OK;
}

int compact_checked(const leann_backend *src, const CompactChecked &c, uint64_t key_offset, leann_backend **out, uint64_t *new_to_old) {
    const size_t n = c.n, live = c.live;
    const GraphView &g = src->g;
    std::vector<uint32_t> o2n(n), n2o(live);
    {
        size_t j = 0;
        for (size_t p = 0; p < n; p++) {
            const bool gone = !c.removed.empty() && ((c.removed[p >> 3] >> (p & 7)) & 1);
            o2n[p] = gone ? LEANN_EMPTY : (uint32_t)j;
            if (!gone) {
                if (j == live) break; // (a bitmap that disagrees with its count: caught below)
                n2o[j++] = (uint32_t)p;
            }
        }
        if (j != live) { leann_set_error("leann_backend_compact: inconsistent graph: the removal bitmap does not hold %zu removals", n - live); return LEANN_ERR_INVALID; }
    }
    if (int rc = leann_internal_check_device(src->device)) return rc;
    HIP_CHECK_RET(hipSetDevice(src->device));
    HIP_CHECK_RET(hipDeviceSynchronize());

    DeviceBuf<uint32_t> d_o2n, d_n2o, d_bad;
    if (d_o2n.alloc(n) || d_n2o.alloc(live) || d_bad.alloc(1)) return LEANN_ERR_DEVICE;
    HIP_CHECK_RET(hipMemcpy(d_o2n, o2n.data(), n * 4, hipMemcpyHostToDevice));
    HIP_CHECK_RET(hipMemcpy(d_n2o, n2o.data(), live * 4, hipMemcpyHostToDevice));
    HIP_CHECK_RET(hipMemset(d_bad, 0, 4));

    // every allocation of the result is a member of the handle: one leann_backend_close frees whatever a failure leaves behind
    HandlePtr h = leann_internal_new_like(src);
    if (key_offset != LEANN_KEY_OFFSET_KEEP) h->key_offset = key_offset;
    h->g.n = live;
    h->g.entry = o2n[g.entry];
    GraphStore &st = h->store;

    // levels first: they say how many upper lists there are; then upper_off on the host
    if (st.levels.alloc(live)) return LEANN_ERR_DEVICE;
    hipLaunchKernelGGL(gather_levels_kernel, dim3((unsigned)((live + 255) / 256)), dim3(256), 0, nullptr, (const uint8_t *)src->store.levels,
                       (const uint32_t *)d_n2o, (uint32_t)live, st.levels.p);
    HIP_CHECK_RET(hipGetLastError());
    std::vector<uint8_t> lv(live);
    HIP_CHECK_RET(hipMemcpy(lv.data(), st.levels, live, hipMemcpyDeviceToHost));
    std::vector<uint32_t> uo(live);
    const uint64_t n_upper = leann_internal_upper_offsets(lv.data(), live, uo.data());
    if (n_upper > src->n_upper_lists || lv[h->g.entry] < g.max_level) {
        leann_set_error("leann_backend_compact: inconsistent graph: %s", n_upper > src->n_upper_lists ? "the levels name more upper lists than the index holds"
                                                                                                      : "the entry point does not reach max_level");
        return LEANN_ERR_INVALID;
    }
    if (int rc = leann_internal_alloc_graph_lists(h.get(), n_upper)) return rc;
    HIP_CHECK_RET(hipMemcpy(st.upper_off, uo.data(), live * 4, hipMemcpyHostToDevice));
    // rows: the result always owns them, at the source's pitch (allocated here: no allocation between the timed launches)
    const size_t pitch = leann_internal_narrow_rows(src) ? (size_t)g.row_bytes : (size_t)g.ld * 4;
    if (pitch == 0 || (pitch & 15) || !g.X) { leann_set_error("leann_backend_compact: rows of %zu bytes cannot be gathered in 16-byte pieces", pitch); return LEANN_ERR_INVALID; }
    DeviceBuf<unsigned char> rows;
    if (rows.alloc(std::max<size_t>(live * pitch, 128))) return LEANN_ERR_DEVICE;
    leann_internal_own_rows(h.get(), std::move(rows));
    if (leann_internal_i8(src)) { // the codes move byte for byte: the columns keep their exponents
        h->i8_exps = src->i8_exps;
        if (int rc = leann_internal_i8_bind_scales(h.get())) return rc;
    }
    const unsigned list_grid = (unsigned)std::min<size_t>((live + 3) / 4, (size_t)1 << 16); // four waves = four nodes per block
    PhaseClock phases;
    phases.mark(0);
    hipLaunchKernelGGL(remap_lists_kernel, dim3(list_grid), dim3(256), 0, nullptr, g.adj0, st.adj0.p, g.M0, (const uint32_t *)d_n2o,
                       (const uint32_t *)d_o2n, (uint32_t)n, (uint32_t)live, (const uint8_t *)nullptr, (const uint32_t *)nullptr,
                       (const uint32_t *)nullptr, (uint64_t)n, d_bad.p);
    HIP_CHECK_RET(hipGetLastError());
    if (n_upper) {
        hipLaunchKernelGGL(remap_lists_kernel, dim3(list_grid), dim3(256), 0, nullptr, g.adjU, st.adjU.p, g.M, (const uint32_t *)d_n2o,
                           (const uint32_t *)d_o2n, (uint32_t)n, (uint32_t)live, (const uint8_t *)st.levels.p, g.upper_off,
                           (const uint32_t *)st.upper_off.p, (uint64_t)src->n_upper_lists, d_bad.p);
        HIP_CHECK_RET(hipGetLastError());
    }
    {
        const uint32_t pieces = (uint32_t)(pitch / 16);
        const uint32_t tile_rows = std::max<uint32_t>(1, GATHER_THREADS * GATHER_UNROLL / pieces);
        const uint64_t tiles = (live + tile_rows - 1) / tile_rows;
        const unsigned grid = (unsigned)std::min<uint64_t>(tiles, 256 * 8 * 4);
        phases.mark(1);
        hipLaunchKernelGGL(gather_rows_kernel, dim3(grid), dim3(GATHER_THREADS), 0, nullptr, reinterpret_cast<const uint4 *>(g.X),
                           reinterpret_cast<uint4 *>(st.rows.p), (const uint32_t *)d_n2o, (uint64_t)live, pieces, tile_rows);
        HIP_CHECK_RET(hipGetLastError());
        phases.mark(2);
    }
    uint32_t bad = 0;
    HIP_CHECK_RET(hipMemcpy(&bad, d_bad, 4, hipMemcpyDeviceToHost));
    HIP_CHECK_RET(hipDeviceSynchronize()); // null-stream work; searches run on non-blocking streams that do not wait for it
    if (bad) {
        leann_set_error("leann_backend_compact: inconsistent graph: a live list names a removed position (n_pending said none); no handle made");
        return LEANN_ERR_INVALID;
    }
    d_o2n.reset(); d_n2o.reset(); d_bad.reset(); // before the planes: the peak stays at source + result
    const auto t0 = std::chrono::steady_clock::now();
    leann_internal_sync_planes(h.get()); // (ends with a device synchronisation when it cuts planes)
    if (phases.on) {
        const double planes_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        const double row_gb = 2.0 * (double)live * (double)pitch / 1e9, list_gb = 2.0 * ((double)live * g.M0 + (double)n_upper * g.M) * 4 / 1e9;
        const float rows_ms = phases.ms(1, 2), lists_ms = phases.ms(0, 1);
        leann_log(LEANN_LOG_INFO, "compact: %zu of %zu positions kept; lists %.3f ms (%.3f GB moved), rows %.3f ms (%.3f GB moved, %.0f GB/s), planes %.3f ms%s",
                  live, n, lists_ms, list_gb, rows_ms, row_gb, rows_ms > 0 ? row_gb / (rows_ms * 1e-3) : 0.0, planes_ms,
                  leann_internal_planes_ready(h.get()) ? "" : " (none cut)");
    }
    if (new_to_old)
        for (size_t j = 0; j < live; j++) new_to_old[j] = src->key_offset + n2o[j];
    *out = h.release();
    return LEANN_OK;
}
} // namespace

extern "C" int leann_backend_compact(const leann_backend *hc, uint64_t key_offset, leann_backend **out, uint64_t *new_to_old) {
    if (out) *out = nullptr;
    if (!hc || !out) { leann_set_error("leann_backend_compact: null argument"); return LEANN_ERR_INVALID; }
    try {
        CompactChecked c;
        if (int rc = check_source(hc, &c)) return rc;
        return compact_checked(hc, c, key_offset, out, new_to_old);
    } catch (const std::exception &e) {
        leann_set_error("leann_backend_compact: %s", e.what());
        return LEANN_ERR_IO;
    }
}

// file twin: open -> consolidate if lists still name removed positions -> compact -> save
extern "C" int leann_backend_compact_index(int backend, size_t dims, const char *index_path_stem, uint64_t *new_to_old, size_t cap,
                                           size_t *n_live) {
    if (n_live) *n_live = 0;
    if (!index_path_stem) { leann_set_error("leann_backend_compact_index: null argument"); return LEANN_ERR_INVALID; }
    leann_backend *h = nullptr;
    int rc = leann_backend_open(index_path_stem, backend, dims, "0", &h);
    if (rc) return rc;
    try {
        const size_t live = leann_backend_live_len(h);
        if (n_live) *n_live = live;
        if (new_to_old && cap < live) {
            leann_set_error("leann_backend_compact_index: the map needs room for %zu positions, cap is %zu", live, cap);
            leann_backend_close(h);
            return LEANN_ERR_INVALID;
        }
        if (h->sharded || h->n_removed == 0) { // nothing removed: identity map, the file stays as it is
            if (h->sharded) { leann_set_error("leann_backend_compact_index: \"%s\" opened as a composite handle", index_path_stem); rc = LEANN_ERR_UNSUPPORTED; }
            else if (new_to_old) for (size_t j = 0; j < live; j++) new_to_old[j] = j;
            leann_backend_close(h);
            return rc;
        }
        const uint32_t e = h->g.entry;
        if (h->n_pending || ((h->removed[e >> 3] >> (e & 7)) & 1)) rc = leann_backend_consolidate(h); // (bf16 / recompute-on: refused there)
        leann_backend *c = nullptr;
        if (rc == LEANN_OK) rc = leann_backend_compact(h, 0, &c, new_to_old);
        if (rc == LEANN_OK) rc = leann_backend_save(c, index_path_stem); // (nothing removed in c: the save deletes the sidecar)
        leann_backend_close(c);
        leann_backend_close(h);
        return rc;
    } catch (const std::exception &ex) {
        leann_backend_close(h);
        leann_set_error("leann_backend_compact_index: %s", ex.what());
        return LEANN_ERR_IO;
    }
}
