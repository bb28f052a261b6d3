// scan_lists.hip — exact top-k over per-query position lists: one launch scans every query's rows.
//
// Per-query filters are the multi-tenant case: query i is answered over its own short list of rows (a tenant's ids, an ACL, a BM25
// posting list, or the set bits of its allow-bitmap).  With one query — or a few — per list there is nothing for a 32 x 32 MFMA tile
// to share: score_mfma_kernel<LIST> (scan.hip) carries one query in a 64-query tile and is launched, selected and synchronised once
// per query.  The work is a segmented, gather-bound GEMV, so this kernel runs it on the vector ALU: one k-ordered chain
// acc = fmaf(x[j], q[j], acc), j ascending from acc = +0, per (query, row) — the chain v_mfma_f32_32x32x2_f32 evaluates (scan.hip),
// over the same zero-padded length (dims rounded up to the 32-wide k-tile), hence the same bits, an underflowed -0 included.
//
// Work units (planned on the host, one flat grid over a small uploaded table): (list, chunk of 256 listed rows, tile of up to QT
// queries that share the list).  The host sorts the queries of a slice by list; a list with one query runs QT = 1, a shared list
// tiles of QT = 8 (the rows of a chunk are then read once per tile, not once per query).
//
// score_lists_kernel<QT, FAST>, 256 threads:
//   positions  thread t checks entry t of the chunk (t < cnt, position < n, live bit) BEFORE any address is formed and parks the
//              position, or LEANN_EMPTY for a skipped entry, in LDS.  No row is addressed through a skipped entry: the general form
//              loads nothing for it, FAST points its unconditional loads at row 0 of the handle and drops the score.
//   staging    score_mfma_kernel's map: thread t loads 16 bytes of row t / 8 (+ 32 per pass, 8 passes) at k offset 4 (t % 8), so one
//              wave instruction reads 8 whole 128-B lines; the next k-tile travels in registers while the current one is consumed;
//              the tile is written transposed into sX[32][256] (32 KB), column ^ 8 ((k >> 2) & 7).  Transposing write: 8 k-groups x 8
//              consecutive rows per wave instruction -> 64 distinct banks.  Read: lane l of a wave reads column (64 w + l) ^ sw(k), a
//              permutation within the wave's 64 columns -> conflict-free.  Up to QT queries go to sQ[QT][32] the same way.
//   arithmetic thread t owns row t and QT accumulators: per k one LDS read of x and QT fmaf whose query operand is the same LDS word
//              for every lane (a broadcast read, fetched four k at a time), never a vector load per lane.
//   selection  fused: per query the 256 keys ~orderable(score) << 32 | position (~0 for a skipped entry) are sorted in LDS
//              (bitonic_sort_lds's network, all queries of the tile under one set of barriers, in the retired row tile) and the
//              first min(top_k, 256) written to cand[query][chunk]; topk_keys_kernel rounds and
//              finalize_scan_kernel (scan.hip; idx = nullptr, as_dist = 1) finish.  The key carries the position itself, so lists need
//              not be sorted, a position listed twice is returned twice, and ties go to the lower position.
//
// Resource budget (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, 256 threads; no instantiation spills or uses scratch):
//   <1, true>    98 VGPRs, 32 SGPRs, LDS 34 176 B, 4 waves / SIMD (four workgroups of four waves per CU)
//   <1, false>  100 VGPRs, 52 SGPRs, LDS 34 176 B, 4 waves / SIMD
//   <8, true>   130 VGPRs, 32 SGPRs, LDS 35 072 B, 3 waves / SIMD
//   <8, false>  132 VGPRs, 52 SGPRs, LDS 35 072 B, 3 waves / SIMD
#include "common.cuh"
#include "../../include/leann_backend.h"
#include "internal.h"
#include "lists_plan.h"
#include <algorithm>
#include <vector>

template <int QT, bool FAST>
__global__ void __launch_bounds__(256) score_lists_kernel(const float *__restrict__ X, uint64_t n, uint32_t d, uint32_t ld,
                                                          const uint8_t *__restrict__ live, const float *__restrict__ Q, uint32_t ldq,
                                                          const ListUnit *__restrict__ units, const uint32_t *__restrict__ qord,
                                                          const uint32_t *__restrict__ lists, uint32_t kk, uint64_t *__restrict__ cand,
                                                          uint32_t cand_len, uint32_t *__restrict__ skipped) {
    constexpr int BK = 32, PASSES = LISTS_ROWS / 32;
    __shared__ __attribute__((aligned(16))) float sX[BK][LISTS_ROWS];
    __shared__ __attribute__((aligned(16))) float sQ[QT][BK];
    __shared__ uint32_t sPos[LISTS_ROWS];
    const int tid = threadIdx.x;
    const ListUnit u = units[blockIdx.x];
    // this thread's entry: range and live checks first, the position only then becomes a row address
    uint32_t pos = LEANN_EMPTY;
    bool beyond = false;
    if ((uint32_t)tid < u.cnt) {
        const uint32_t p = lists[u.off + tid];
        beyond = p >= n;
        if (!beyond && (!live || ((live[p >> 3] >> (p & 7)) & 1))) pos = p;
    }
    sPos[tid] = pos;
    const int n_beyond = __syncthreads_count(beyond); // (also publishes sPos)
    if (skipped && n_beyond && (uint32_t)tid < u.nqt) atomicAdd(&skipped[qord[u.q0 + tid]], (uint32_t)n_beyond);

    const int sr = tid >> 3, kq = (tid & 7) * 4, sw_w = 8 * (tid & 7); // (k >> 2) & 7 of this thread's four k is tid & 7
    const bool qthread = tid < QT * 8;
    const uint32_t qslot = min((uint32_t)sr, u.nqt - 1); // a tile's unused query slots repeat its last query; their sums are dropped
    const float *qrow = Q + (size_t)qord[u.q0 + qslot] * ldq;
    const bool xvec = ((ld & 3) == 0) && ((reinterpret_cast<uintptr_t>(X) & 15) == 0);
    const bool qvec = ((ldq & 3) == 0) && ((reinterpret_cast<uintptr_t>(Q) & 15) == 0);
    auto load4 = [&](const float *base, bool ok, bool vec, uint32_t k, uint32_t lim) -> float4 {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok) {
            if (vec && k + 3 < lim) v = *reinterpret_cast<const float4 *>(base + k);
            else {
                if (k + 0 < lim) v.x = base[k + 0];
                if (k + 1 < lim) v.y = base[k + 1];
                if (k + 2 < lim) v.z = base[k + 2];
                if (k + 3 < lim) v.w = base[k + 3];
            }
        }
        return v;
    };
    float4 xv[PASSES], qv = make_float4(0.f, 0.f, 0.f, 0.f);
    uint32_t xrow[PASSES];
#pragma unroll
    for (int p = 0; p < PASSES; p++) xrow[p] = sPos[sr + 32 * p];
    const float *xp[PASSES]; // FAST: a skipped entry's loads go to row 0 (n > 0: the host picks the general form for an empty handle)
    if constexpr (FAST) {
#pragma unroll
        for (int p = 0; p < PASSES; p++) xp[p] = X + (size_t)(xrow[p] == LEANN_EMPTY ? 0u : xrow[p]) * ld + kq;
    }
    auto gload = [&](uint32_t k0) {
        if constexpr (FAST) {
#pragma unroll
            for (int p = 0; p < PASSES; p++) xv[p] = *reinterpret_cast<const float4 *>(xp[p] + k0);
            if (qthread) qv = *reinterpret_cast<const float4 *>(qrow + kq + k0);
        } else {
#pragma unroll
            for (int p = 0; p < PASSES; p++) xv[p] = load4(X + (size_t)(xrow[p] == LEANN_EMPTY ? 0u : xrow[p]) * ld, xrow[p] != LEANN_EMPTY, xvec, k0 + kq, d);
            if (qthread) qv = load4(qrow, true, qvec, k0 + kq, d);
        }
    };
    float acc[QT];
#pragma unroll
    for (int j = 0; j < QT; j++) acc[j] = 0.f;
    gload(0);
    for (uint32_t k0 = 0; k0 < d; k0 += BK) {
#pragma unroll
        for (int e = 0; e < 4; e++) {
#pragma unroll
            for (int p = 0; p < PASSES; p++) sX[kq + e][(sr + 32 * p) ^ sw_w] = e == 0 ? xv[p].x : e == 1 ? xv[p].y : e == 2 ? xv[p].z : xv[p].w;
        }
        if (qthread) *reinterpret_cast<float4 *>(&sQ[sr][kq]) = qv;
        __syncthreads();
        if (k0 + BK < d) gload(k0 + BK);
#pragma unroll
        for (int k = 0; k < BK; k++) {
            const float x = sX[k][tid ^ (8 * ((k >> 2) & 7))];
#pragma unroll
            for (int j = 0; j < QT; j++) acc[j] = fmaf(x, sQ[j][k], acc[j]);
        }
        __syncthreads();
    }
    // fused selection: the chunk's 256 keys of each query, sorted; the first kk go to the query's slot of this chunk
    // (keys[QT][256] takes the place of sX, which the k loop's last barrier has retired; bitonic_sort_lds's network — common.cuh —
    // runs over the nqt segments at once, so a tile pays one set of barriers, not one per query)
    uint64_t *keys = reinterpret_cast<uint64_t *>(&sX[0][0]);
    static_assert(sizeof(uint64_t) * QT * LISTS_ROWS <= sizeof(sX), "the key segments live in the row tile");
#pragma unroll
    for (int j = 0; j < QT; j++) keys[j * LISTS_ROWS + tid] = pos != LEANN_EMPTY ? ((uint64_t)(~f32_orderable(acc[j])) << 32) | pos : ~0ull;
    const int n_cmp = (int)u.nqt * (int)(LISTS_ROWS / 2);
    for (int size = 2; size <= (int)LISTS_ROWS; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int i = tid; i < n_cmp; i += 256) {
                uint64_t *seg = keys + (i >> 7) * LISTS_ROWS;
                const int c = i & 127, lo = 2 * c - (c & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const uint64_t a = seg[lo], b = seg[hi];
                if ((a > b) == up) { seg[lo] = b; seg[hi] = a; }
            }
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < u.nqt * kk; i += 256) {
        const uint32_t j = i / kk, r = i - j * kk;
        cand[(size_t)qord[u.q0 + j] * cand_len + (size_t)u.chunk * kk + r] = keys[j * LISTS_ROWS + r];
    }
}

// One slice of queries [0, nq) (the caller has offset every per-query pointer): plan, upload, score + select, reduce.
static int lists_slice(const float *X, size_t n, size_t dims, size_t ld, const uint8_t *d_live, const float *Q, size_t nq, uint32_t k,
                       const uint64_t *list_off, const uint32_t *d_lists, const uint32_t *q_list, size_t q_base, size_t max_chunks,
                       uint64_t key_offset, uint64_t *d_keys, float *d_dists, uint32_t *d_counts, uint32_t *d_skipped, hipStream_t st) {
    const uint32_t kk = std::min<uint32_t>(k, LISTS_ROWS);
    const size_t m = max_chunks * kk, cand_len = std::max<size_t>(m, k);
    // queries sorted by list (stable); units of lone queries first (QT = 1), then the tiles of shared lists (lists_plan.h)
    const ListsPlan plan = lists_plan_units(nq, list_off, q_list, q_base);
    const std::vector<uint32_t> &ord = plan.ord;
    const std::vector<ListUnit> &table = plan.table;
    const size_t n_units = table.size(), n_lone = plan.n_lone, n_tiled = plan.n_tiled();
    if (n_units >= (1ull << 31)) { leann_set_error("exact lists search: %zu work units in one slice", n_units); return LEANN_ERR_INVALID; }
    ScratchLease<uint64_t> candA, candB;
    ScratchLease<ListUnit> d_units;
    ScratchLease<uint32_t> d_ord;
    struct SyncFirst { // (declared after the leases, so it runs before them) nothing may still be running on a block that goes back
        hipStream_t st;
        ~SyncFirst() { (void)hipStreamSynchronize(st); }
    } sync_first{st};
    if (int e = candA.acquire(nq * cand_len)) return e;
    if (int e = candB.acquire(nq * cand_len)) return e;
    if (int e = d_units.acquire(std::max<size_t>(n_units, 1))) return e;
    if (int e = d_ord.acquire(nq)) return e;
    HIP_CHECK_RET(hipMemsetAsync(candA, 0xFF, sizeof(uint64_t) * nq * cand_len, st));
    if (d_skipped) HIP_CHECK_RET(hipMemsetAsync(d_skipped, 0, 4 * nq, st));
    HIP_CHECK_RET(hipMemcpyAsync(d_ord, ord.data(), 4 * nq, hipMemcpyHostToDevice, st));
    if (n_units) HIP_CHECK_RET(hipMemcpyAsync(d_units, table.data(), sizeof(ListUnit) * n_units, hipMemcpyHostToDevice, st));
    const bool fast = dims % 32 == 0 && ld % 4 == 0 && n > 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0 && (reinterpret_cast<uintptr_t>(Q) & 15) == 0;
#define LEANN_LISTS_LAUNCH(QT_, FAST_, first, count)                                                                                        \
    hipLaunchKernelGGL((score_lists_kernel<QT_, FAST_>), dim3((unsigned)(count)), dim3(256), 0, st, X, (uint64_t)n, (uint32_t)dims,          \
                       (uint32_t)ld, d_live, Q, (uint32_t)dims, d_units.p + (first), d_ord.p, d_lists, kk, candA.p, (uint32_t)cand_len,      \
                       d_skipped)
    if (n_lone) { if (fast) LEANN_LISTS_LAUNCH(1, true, 0, n_lone); else LEANN_LISTS_LAUNCH(1, false, 0, n_lone); }
    if (n_tiled) {
        if (fast) LEANN_LISTS_LAUNCH(LISTS_QT, true, n_lone, n_tiled);
        else LEANN_LISTS_LAUNCH(LISTS_QT, false, n_lone, n_tiled);
    }
#undef LEANN_LISTS_LAUNCH
    HIP_CHECK_RET(hipGetLastError());
    if (int rc = leann_internal_keys_finish(candA, candB, cand_len, m, max_chunks <= 1, nq, k, key_offset, d_keys, d_dists, d_counts, st, nullptr, 1))
        return rc;
    HIP_CHECK_RET(hipStreamSynchronize(st)); // (the host tables above are read by the copies until here)
    return LEANN_OK;
}

int leann_internal_exact_lists(const float *d_rows, size_t n, size_t dims, size_t ld, const uint8_t *d_live, const float *d_queries, size_t nq,
                               size_t top_k, const uint64_t *list_off, const uint32_t *d_lists, const uint32_t *q_list, uint64_t key_offset,
                               uint64_t *d_keys, float *d_dists, uint32_t *d_counts, uint32_t *d_skipped, hipStream_t st) {
    if (top_k == 0 || top_k > SEG / 2 || n >= (1ull << 32)) {
        leann_set_error("exact lists search: top_k must be in [1, %d] and the index smaller than 2^32 rows (top_k=%zu n=%zu)", SEG / 2, top_k, n);
        return LEANN_ERR_INVALID;
    }
    const uint32_t k = (uint32_t)top_k;
    // query slices: the two candidate buffers of a slice stay within the scan pool's 64 MiB blocks (lists_plan.h)
    for (size_t q0 = 0; q0 < nq;) {
        size_t max_chunks = 0;
        const size_t q1 = lists_plan_slice_end(q0, nq, k, list_off, q_list, &max_chunks);
        if (int rc = lists_slice(d_rows, n, dims, ld, d_live, d_queries + q0 * dims, q1 - q0, k, list_off, d_lists, q_list, q0, max_chunks, key_offset,
                                 d_keys + q0 * top_k, d_dists + q0 * top_k, d_counts + q0, d_skipped ? d_skipped + q0 : nullptr, st))
            return rc;
        q0 = q1;
    }
    return LEANN_OK;
}

// what every lists call asks of list_off and q_list (HOST arrays), naming the argument; `lists` may be null only when every list is empty
int leann_internal_lists_check_offsets(const char *who, size_t nq, const uint64_t *list_off, const void *lists, size_t n_lists, const uint32_t *q_list) {
    if (list_off[0] != 0) { leann_set_error("%s: list_off[0] = %llu, not 0", who, (unsigned long long)list_off[0]); return LEANN_ERR_INVALID; }
    for (size_t l = 0; l < n_lists; l++)
        if (list_off[l + 1] < list_off[l] || list_off[l + 1] - list_off[l] >= (1ull << 31)) {
            leann_set_error("%s: list_off[%zu] = %llu after %llu: offsets must be monotone and a list shorter than 2^31 entries", who, l + 1,
                            (unsigned long long)list_off[l + 1], (unsigned long long)list_off[l]);
            return LEANN_ERR_INVALID;
        }
    if (list_off[n_lists] && !lists) { leann_set_error("%s: null lists", who); return LEANN_ERR_INVALID; }
    if (!q_list && n_lists != nq) {
        leann_set_error("%s: q_list is null, so query i takes list i, but n_lists = %zu and nq = %zu", who, n_lists, nq);
        return LEANN_ERR_INVALID;
    }
    for (size_t i = 0; q_list && i < nq; i++)
        if (q_list[i] >= n_lists) { leann_set_error("%s: q_list[%zu] = %u, n_lists = %zu", who, i, q_list[i], n_lists); return LEANN_ERR_INVALID; }
    return LEANN_OK;
}

// ---- C ABI (include/leann_backend.h) -------------------------------------------------------------------------------------------------
// every refusal happens here, on the host, before any device work
static int lists_check(const char *who, const leann_backend *h, const void *queries, size_t nq, size_t top_k, const uint64_t *list_off,
                       const void *lists, size_t n_lists, const uint32_t *q_list, const void *keys, const void *dists, const void *counts) {
    const char *null_arg = !h ? "h" : !list_off ? "list_off" : !nq ? nullptr : !queries ? "queries" : !keys ? "keys" : !dists ? "dists" : !counts ? "counts" : nullptr;
    if (null_arg) { leann_set_error("%s: null %s", who, null_arg); return LEANN_ERR_INVALID; }
    if (h->sharded) {
        leann_set_error("%s: lists hold positions local to one handle and this handle is a composite one; pass allow-bitmaps over global "
                        "positions (leann_backend_search_filtered_exact_batch), which are sliced per shard", who);
        return LEANN_ERR_UNSUPPORTED;
    }
    if (h->g.feat_h) {
        leann_set_error("exact filtered search needs stored vectors; this index recomputes them from features (use leann_recompute_search_batch_device with an allow mask)");
        return LEANN_ERR_UNSUPPORTED;
    }
    if (leann_internal_narrow_rows(h)) {
        leann_set_error("exact filtered search scans f32 rows; this index stores %s rows (use the filtered walk: mode 0, or mode 2 which picks it)",
                        leann_internal_row_name(h));
        return LEANN_ERR_UNSUPPORTED;
    }
    if (top_k == 0 || top_k > SEG / 2) { leann_set_error("%s: top_k = %zu is outside [1, %d]", who, top_k, SEG / 2); return LEANN_ERR_INVALID; }
    return leann_internal_lists_check_offsets(who, nq, list_off, lists, n_lists, q_list);
}

extern "C" int leann_backend_search_exact_lists_batch_device(const leann_backend *h, const float *d_queries, size_t nq, size_t top_k,
                                                             const uint64_t *list_off, const uint32_t *d_lists, size_t n_lists,
                                                             const uint32_t *q_list, uint64_t *d_keys, float *d_dists, uint32_t *d_counts,
                                                             uint32_t *d_skipped, void *stream) {
    if (int rc = lists_check("leann_backend_search_exact_lists_batch_device", h, d_queries, nq, top_k, list_off, d_lists, n_lists, q_list, d_keys,
                             d_dists, d_counts))
        return rc;
    if (nq == 0) return LEANN_OK;
    HIP_CHECK_RET(hipSetDevice(h->device));
    return leann_internal_exact_lists(h->g.X, h->g.n, h->g.d, h->g.ld, h->d_live, d_queries, nq, top_k, list_off, d_lists, q_list, h->key_offset,
                                      d_keys, d_dists, d_counts, d_skipped, (hipStream_t)stream);
}

extern "C" int leann_backend_search_exact_lists_batch(const leann_backend *h, const float *queries, size_t nq, size_t top_k,
                                                      const uint64_t *list_off, const uint32_t *lists, size_t n_lists, const uint32_t *q_list,
                                                      uint64_t *keys, float *dists, uint32_t *counts, uint32_t *skipped) {
    if (int rc = lists_check("leann_backend_search_exact_lists_batch", h, queries, nq, top_k, list_off, lists, n_lists, q_list, keys, dists, counts))
        return rc;
    if (nq == 0) return LEANN_OK;
    HIP_CHECK_RET(hipSetDevice(h->device));
    const size_t d = h->g.d, total = (size_t)list_off[n_lists];
    DeviceBuf<float> d_q, d_dists;
    DeviceBuf<uint64_t> d_keys;
    DeviceBuf<uint32_t> d_lists, d_counts, d_skipped;
    if (int rc = d_q.alloc(nq * d)) return rc;
    if (int rc = d_lists.alloc(total)) return rc;
    if (int rc = d_keys.alloc(nq * top_k)) return rc;
    if (int rc = d_dists.alloc(nq * top_k)) return rc;
    if (int rc = d_counts.alloc(nq)) return rc;
    if (int rc = d_skipped.alloc(nq)) return rc;
    HIP_CHECK_RET(hipMemcpy(d_q, queries, nq * d * 4, hipMemcpyHostToDevice));
    if (total) HIP_CHECK_RET(hipMemcpy(d_lists, lists, total * 4, hipMemcpyHostToDevice));
    if (int rc = leann_internal_exact_lists(h->g.X, h->g.n, d, h->g.ld, h->d_live, d_q, nq, top_k, list_off, d_lists, q_list, h->key_offset, d_keys,
                                            d_dists, d_counts, d_skipped, nullptr))
        return rc;
    HIP_CHECK_RET(hipMemcpy(keys, d_keys, nq * top_k * 8, hipMemcpyDeviceToHost));
    HIP_CHECK_RET(hipMemcpy(dists, d_dists, nq * top_k * 4, hipMemcpyDeviceToHost));
    HIP_CHECK_RET(hipMemcpy(counts, d_counts, nq * 4, hipMemcpyDeviceToHost));
    if (skipped) HIP_CHECK_RET(hipMemcpy(skipped, d_skipped, nq * 4, hipMemcpyDeviceToHost));
    return LEANN_OK;
}
