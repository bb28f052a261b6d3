// scan_lists_i8.hip — int8 rows: exact search over per-query position lists and per-query allow-bitmaps (include/leann_backend.h
// "exhaustive search on int8 rows, per query"): leann_backend_search_flat_lists_batch[_device] and
// leann_backend_search_flat_filtered_batch[_device].
//
// Query i is answered over its own rows (a tenant's ids, an ACL, the set bits of its bitmap).  With one query — or a few — per row
// list the 32 x 32 integer MFMA tile of scan_i8.hip has nothing to share, as scan_lists.hip says of the f32 one: the work is a
// segmented, gather-bound GEMV.  On int8 rows that GEMV runs on the vector ALU's packed 8-bit dot product, v_dot4c_i32_i8
// (__builtin_amdgcn_sdot4, signed x signed — the codes are in [-127, 127]): four multiply-adds per instruction into an int32 that
// cannot overflow (127^2 * 4096 < 2^31).  The sum is order-free, so the store's element permutation is never undone: the query codes
// are written in store order (quantize_queries_i8_kernel) and the kernel multiplies bytes as they lie.  The screen's candidates then
// get the walk's distance from rescore_i8_kernel<T> (scan_i8.hip), exactly as the flat search's do.
//
// Work units (lists_plan.h, one flat grid over a small uploaded table): (list, chunk of 256 listed rows, tile of up to QT queries that
// share the list); QT = 1 for a list with one query, QT = 8 for a shared one (the rows of a chunk are read once per tile).
//
// score_lists_i8_kernel<QT>, 256 threads:
//   positions  thread t checks entry t of the chunk (t < cnt, position < n, live bit) BEFORE any address is formed and parks the
//              position, or LEANN_EMPTY for a skipped entry, in LDS; __syncthreads_count gives the beyond-n count of the chunk, added
//              to d_skipped of every query of the tile.  A skipped entry's loads point at row 0 (the host never launches for n == 0)
//              and its score is dropped.
//   staging    a k-tile is ONE 128-B line per row (128 codes).  Thread t loads 16 B of row t / 8 (+ 32 per pass, 8 passes) at byte
//              16 (t % 8): a wave instruction reads eight whole lines.  The next k-tile travels in registers while the current one is
//              consumed.  Rows are whole zero-padded lines and the query codes are padded with zeros: no tail, no alignment branch,
//              no general form.  The lines go into LDS as they lie, sX[256][8] 16-B columns (32 KiB), column c of row r at slot
//              c ^ sw(r), sw = scan_i8.hip's flat_sw; the <= QT code rows of the tile into sQ[QT][8] (a tile's unused slots repeat its
//              last query; their sums are dropped).
//   arithmetic thread t owns row t and QT int32 accumulators: per k-tile eight ds_read_b128 of its row and, per dword, QT packed dots
//              whose query operand is the same LDS address for every lane — a broadcast read, never a vector load per lane.
//   selection  fused, as in score_lists_kernel: per query the 256 keys ~orderable((float)s) << 32 | position (~0 for a skipped entry)
//              are sorted in the retired row tile under one set of barriers and the first min(fetch_k, 256) written to
//              cand[query][chunk]; leann_internal_keys_finish (idx null, key offset 0) reduces the chunks to the fetch_k candidate
//              positions and their count.  (float)s is v_cvt_f32_i32, round to nearest even, as the flat screen's.
//
// Banks (scan_i8.hip's argument, the roles of its two accesses unchanged).  Compute read: consecutive lanes read the SAME column of
// consecutive rows, 128 B apart; over any aligned 8 rows sw takes 8 distinct values, so 8 lanes cover the 32 banks of a line exactly
// once, and over any aligned 16 rows the pairs (r & 1, sw(r)) are distinct, so 16 lanes cover 64 banks once: conflict-free whether
// the LDS serves 128 B or 256 B per clock.  Staging write: 8 lanes write the 8 slots of one row — one whole line —, the next 8 lanes
// the next row: conflict-free for the same reason.  (Reasoned from the layout; the LDS conflict counter was not read.)
//
// Resource budget (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, 256 threads; nothing spills, no scratch instruction):
//   <1>    92 VGPRs, 0 AGPRs, 32 SGPRs, LDS 34 176 B, 4 waves / SIMD (four workgroups of four waves per CU)
//   <8>   128 VGPRs, 0 AGPRs, 32 SGPRs, LDS 35 072 B, 4 waves / SIMD
// The ISA holds 32 and 256 v_dot4c_i32_i8 (one k-tile: 8 columns x 4 dwords x QT) and no scratch instruction.
#include "common.cuh"
#include "../../include/leann_backend.h"
#include "internal.h"
#include "lists_plan.h"
#include <algorithm>
#include <vector>

typedef int i32x4 __attribute__((ext_vector_type(4)));
// scan_i8.hip's flat_sw: 8 distinct values over any aligned 8 rows, the pairs (r & 1, sw(r)) distinct over any aligned 16
__device__ __forceinline__ uint32_t lists_sw(uint32_t r) { return ((r >> 1) & 7u) ^ ((r & 1u) << 2); }

// Qc: the slice's query codes, [.. x ldb] in store order; qord: the slice's queries sorted by list; cand [query][cand_len].
template <int QT>
__global__ void __launch_bounds__(256) score_lists_i8_kernel(const int8_t *__restrict__ X, uint64_t n, uint32_t ldb,
                                                             const uint8_t *__restrict__ live, const int8_t *__restrict__ Qc,
                                                             const ListUnit *__restrict__ units, const uint32_t *__restrict__ qord,
                                                             const uint32_t *__restrict__ lists, uint32_t kk, uint64_t *__restrict__ cand,
                                                             uint32_t cand_len, uint32_t *__restrict__ skipped) {
    constexpr int PASSES = LISTS_ROWS / 32;
    __shared__ i32x4 sX[LISTS_ROWS * 8];
    __shared__ i32x4 sQ[QT * 8];
    __shared__ uint32_t sPos[LISTS_ROWS];
    const uint32_t tid = threadIdx.x;
    const ListUnit u = units[blockIdx.x];
    // this thread's entry: range and live checks first, the position only then becomes a row address
    uint32_t pos = LEANN_EMPTY;
    bool beyond = false;
    if (tid < u.cnt) {
        const uint32_t p = lists[u.off + tid];
        beyond = p >= n;
        if (!beyond && (!live || ((live[p >> 3] >> (p & 7)) & 1))) pos = p;
    }
    sPos[tid] = pos;
    const int n_beyond = __syncthreads_count(beyond); // (also publishes sPos)
    if (skipped && n_beyond && tid < u.nqt) atomicAdd(&skipped[qord[u.q0 + tid]], (uint32_t)n_beyond);

    const uint32_t sr = tid >> 3, sc = tid & 7; // staging: row sr (+ 32 per pass) / query sr, 16-B column sc
    const bool qthread = tid < QT * 8;
    const int8_t *xp[PASSES];
#pragma unroll
    for (int p = 0; p < PASSES; p++) {
        const uint32_t row = sPos[sr + 32 * p];
        xp[p] = X + (size_t)(row == LEANN_EMPTY ? 0u : row) * ldb + 16 * sc;
    }
    const int8_t *qp = Qc + (size_t)qord[u.q0 + min(sr, u.nqt - 1)] * ldb + 16 * sc; // (read by the query threads only)
    i32x4 xv[PASSES], qv = {0, 0, 0, 0};
    auto gload = [&](uint32_t k0) {
#pragma unroll
        for (int p = 0; p < PASSES; p++) xv[p] = *reinterpret_cast<const i32x4 *>(xp[p] + k0);
        if (qthread) qv = *reinterpret_cast<const i32x4 *>(qp + k0);
    };
    const uint32_t wslot = sc ^ lists_sw(sr); // (sw(sr + 32 p) == sw(sr))
    const uint32_t rsw = lists_sw(tid);
    int acc[QT];
#pragma unroll
    for (int j = 0; j < QT; j++) acc[j] = 0;
    gload(0);
    for (uint32_t k0 = 0; k0 < ldb; k0 += 128) {
#pragma unroll
        for (int p = 0; p < PASSES; p++) sX[(sr + 32 * p) * 8 + wslot] = xv[p];
        if (qthread) sQ[sr * 8 + sc] = qv;
        __syncthreads();
        if (k0 + 128 < ldb) gload(k0 + 128);
#pragma unroll
        for (uint32_t c = 0; c < 8; c++) {
            const i32x4 x = sX[tid * 8 + (c ^ rsw)];
#pragma unroll
            for (int j = 0; j < QT; j++) {
                const i32x4 q = sQ[j * 8 + c];
#pragma unroll
                for (int e = 0; e < 4; e++) acc[j] = __builtin_amdgcn_sdot4(x[e], q[e], acc[j], false);
            }
        }
        __syncthreads();
    }
    // fused selection: the chunk's 256 keys of each query, sorted; the first kk go to the query's slot of this chunk (keys[QT][256]
    // takes the place of sX, which the k loop's last barrier has retired; score_lists_kernel's network over the nqt segments at once)
    uint64_t *keys = reinterpret_cast<uint64_t *>(sX);
    static_assert(sizeof(uint64_t) * QT * LISTS_ROWS <= sizeof(sX), "the key segments live in the row tile");
#pragma unroll
    for (int j = 0; j < QT; j++) keys[j * LISTS_ROWS + tid] = pos != LEANN_EMPTY ? ((uint64_t)(~f32_orderable((float)acc[j])) << 32) | pos : ~0ull;
    const int n_cmp = (int)u.nqt * (int)(LISTS_ROWS / 2);
    for (int size = 2; size <= (int)LISTS_ROWS; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int i = (int)tid; i < n_cmp; i += 256) {
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

// One slice of queries [0, nq) (the caller has offset every per-query pointer): plan, upload, score + select, reduce to the fetch_k = k
// candidate positions of each query (candK, their scores candS, their number candC).
static int lists_i8_slice(const int8_t *X, size_t n, uint32_t ldb, const uint8_t *d_live, const int8_t *Qc, size_t nq, uint32_t k,
                          const uint64_t *list_off, const uint32_t *d_lists, const uint32_t *q_list, size_t q_base, size_t max_chunks,
                          uint64_t *candK, float *candS, uint32_t *candC, uint32_t *d_skipped, hipStream_t st) {
    const uint32_t kk = std::min<uint32_t>(k, LISTS_ROWS);
    const size_t m = max_chunks * kk, cand_len = std::max<size_t>(m, k);
    const ListsPlan plan = lists_plan_units(nq, list_off, q_list, q_base);
    const size_t n_units = plan.table.size();
    if (n_units >= (1ull << 31)) { leann_set_error("flat lists search: %zu work units in one slice", n_units); return LEANN_ERR_INVALID; }
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
    HIP_CHECK_RET(hipMemcpyAsync(d_ord, plan.ord.data(), 4 * nq, hipMemcpyHostToDevice, st));
    if (n_units) HIP_CHECK_RET(hipMemcpyAsync(d_units, plan.table.data(), sizeof(ListUnit) * n_units, hipMemcpyHostToDevice, st));
    if (plan.n_lone)
        hipLaunchKernelGGL(score_lists_i8_kernel<1>, dim3((unsigned)plan.n_lone), dim3(256), 0, st, X, (uint64_t)n, ldb, d_live, Qc, d_units.p, d_ord.p,
                           d_lists, kk, candA.p, (uint32_t)cand_len, d_skipped);
    if (plan.n_tiled())
        hipLaunchKernelGGL(score_lists_i8_kernel<LISTS_QT>, dim3((unsigned)plan.n_tiled()), dim3(256), 0, st, X, (uint64_t)n, ldb, d_live, Qc,
                           d_units.p + plan.n_lone, d_ord.p, d_lists, kk, candA.p, (uint32_t)cand_len, d_skipped);
    HIP_CHECK_RET(hipGetLastError());
    // keys = positions, no key offset yet; the screen's scores are not part of the answer
    if (int rc = leann_internal_keys_finish(candA, candB, cand_len, m, max_chunks <= 1, nq, k, 0, candK, candS, candC, st, nullptr, 0)) return rc;
    HIP_CHECK_RET(hipStreamSynchronize(st)); // (the plan's host tables are read by the copies until here)
    return LEANN_OK;
}

// The search on a checked int8 handle with n > 0 rows: codes, per slice the screen, the walk's distance on the candidates.  d_live: the
// mask a listed position must pass (null: none, or the lists hold live positions only).  Returns with `st` synchronised.
static int flat_lists_i8_run(const leann_backend *h, const float *d_queries, size_t nq, size_t top_k, size_t fetch_k, const uint64_t *list_off,
                             const uint32_t *d_lists, const uint32_t *q_list, const uint8_t *d_live, uint64_t *d_keys, float *d_dists,
                             uint32_t *d_counts, uint32_t *d_skipped, hipStream_t st) {
    const GraphView &g = h->g;
    const uint32_t ldb = g.row_bytes, k = (uint32_t)fetch_k;
    ScratchLease<int8_t> Qc;
    ScratchLease<uint32_t> bad, candC;
    ScratchLease<uint64_t> candK;
    ScratchLease<float> candS;
    struct SyncFirst {
        hipStream_t st;
        ~SyncFirst() { (void)hipStreamSynchronize(st); }
    } sync_first{st};
    if (int e = Qc.acquire(leann_internal_i8_query_rows(nq) * ldb)) return e;
    if (int e = bad.acquire(nq)) return e;
    if (int e = candK.acquire(nq * k)) return e;
    if (int e = candS.acquire(nq * k)) return e;
    if (int e = candC.acquire(nq)) return e;
    if (int rc = leann_internal_quantize_queries_i8(h, d_queries, nq, Qc, bad, st)) return rc;
    for (size_t q0 = 0; q0 < nq;) {
        size_t max_chunks = 0;
        const size_t q1 = lists_plan_slice_end(q0, nq, k, list_off, q_list, &max_chunks);
        if (int rc = lists_i8_slice(reinterpret_cast<const int8_t *>(g.X), g.n, ldb, d_live, Qc.p + q0 * ldb, q1 - q0, k, list_off, d_lists, q_list, q0,
                                    max_chunks, candK.p + q0 * k, candS.p + q0 * k, candC.p + q0, d_skipped ? d_skipped + q0 : nullptr, st))
            return rc;
        q0 = q1;
    }
    if (int rc = leann_internal_rescore_i8(h, d_queries, nq, candK, candC, bad, k, (uint32_t)top_k, d_keys, d_dists, d_counts, st)) return rc;
    HIP_CHECK_RET(hipStreamSynchronize(st));
    return LEANN_OK;
}

// ---- C ABI (include/leann_backend.h) -------------------------------------------------------------------------------------------------
// every refusal happens here, on the host, before any device work: null arguments and k, then the lists (the handle is not read
// before these), then the handles the screen is not defined for
static int flat_lists_check(const char *who, const leann_backend *h, const void *queries, size_t nq, size_t top_k, size_t fetch_k,
                            const uint64_t *list_off, const void *lists, size_t n_lists, const uint32_t *q_list, const void *keys, const void *dists,
                            const void *counts) {
    if (int rc = leann_internal_flat_check_args(who, h, queries, nq, top_k, fetch_k, keys, dists, counts)) return rc;
    if (!list_off) { leann_set_error("%s: null list_off", who); return LEANN_ERR_INVALID; }
    if (int rc = leann_internal_lists_check_offsets(who, nq, list_off, lists, n_lists, q_list)) return rc;
    return leann_internal_flat_check_handle(who, h, nq);
}
// an empty index: no candidates, and every listed position lies beyond it
static void empty_index_skipped(const uint64_t *list_off, const uint32_t *q_list, size_t nq, std::vector<uint32_t> *out) {
    out->resize(nq);
    for (size_t i = 0; i < nq; i++) {
        const size_t l = lists_plan_list_of(q_list, i);
        (*out)[i] = (uint32_t)(list_off[l + 1] - list_off[l]);
    }
}

extern "C" int leann_backend_search_flat_lists_batch_device(const leann_backend *h, const float *d_queries, size_t nq, size_t top_k, size_t fetch_k,
                                                            const uint64_t *list_off, const uint32_t *d_lists, size_t n_lists,
                                                            const uint32_t *q_list, uint64_t *d_keys, float *d_dists, uint32_t *d_counts,
                                                            uint32_t *d_skipped, void *stream) {
    if (int rc = flat_lists_check("leann_backend_search_flat_lists_batch_device", h, d_queries, nq, top_k, fetch_k, list_off, d_lists, n_lists, q_list,
                                  d_keys, d_dists, d_counts))
        return rc;
    if (nq == 0) return LEANN_OK;
    HIP_CHECK_RET(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    if (h->g.n == 0) {
        std::vector<uint32_t> sk;
        empty_index_skipped(list_off, q_list, nq, &sk);
        HIP_CHECK_RET(hipMemsetAsync(d_counts, 0, nq * 4, st));
        if (d_skipped) HIP_CHECK_RET(hipMemcpyAsync(d_skipped, sk.data(), nq * 4, hipMemcpyHostToDevice, st));
        HIP_CHECK_RET(hipStreamSynchronize(st));
        return LEANN_OK;
    }
    return flat_lists_i8_run(h, d_queries, nq, top_k, fetch_k, list_off, d_lists, q_list, h->d_live, d_keys, d_dists, d_counts, d_skipped, st);
}

extern "C" int leann_backend_search_flat_lists_batch(const leann_backend *h, const float *queries, size_t nq, size_t top_k, size_t fetch_k,
                                                     const uint64_t *list_off, const uint32_t *lists, size_t n_lists, const uint32_t *q_list,
                                                     uint64_t *keys, float *dists, uint32_t *counts, uint32_t *skipped) {
    if (int rc = flat_lists_check("leann_backend_search_flat_lists_batch", h, queries, nq, top_k, fetch_k, list_off, lists, n_lists, q_list, keys, dists,
                                  counts))
        return rc;
    if (nq == 0) return LEANN_OK;
    if (h->g.n == 0) { // nothing to search: answered on the host
        std::vector<uint32_t> sk;
        empty_index_skipped(list_off, q_list, nq, &sk);
        for (size_t i = 0; i < nq; i++) {
            counts[i] = 0;
            if (skipped) skipped[i] = sk[i];
        }
        return LEANN_OK;
    }
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
    if (int rc = flat_lists_i8_run(h, d_q, nq, top_k, fetch_k, list_off, d_lists, q_list, h->d_live, d_keys, d_dists, d_counts, d_skipped, nullptr))
        return rc;
    HIP_CHECK_RET(hipMemcpy(keys, d_keys, nq * top_k * 8, hipMemcpyDeviceToHost));
    HIP_CHECK_RET(hipMemcpy(dists, d_dists, nq * top_k * 4, hipMemcpyDeviceToHost));
    HIP_CHECK_RET(hipMemcpy(counts, d_counts, nq * 4, hipMemcpyDeviceToHost));
    if (skipped) HIP_CHECK_RET(hipMemcpy(skipped, d_skipped, nq * 4, hipMemcpyDeviceToHost));
    return LEANN_OK;
}

// One bitmap per query: live AND allow (consolidate.hip), the bitmaps of a batch into one CSR of ascending position lists in a single
// pass (scan.hip), the lists search over it.  The batch is cut so that even all-ones bitmaps stay within 2^28 list entries at a time,
// as leann_internal_filtered_exact cuts it.  One bitmap for the batch, or none: the flat search as it is.
extern "C" int leann_backend_search_flat_filtered_batch_device(const leann_backend *hc, const float *d_queries, size_t nq, size_t top_k,
                                                               size_t fetch_k, const uint8_t *d_allow, size_t allow_stride, uint64_t *d_keys,
                                                               float *d_dists, uint32_t *d_counts, void *stream) {
    const char *who = "leann_backend_search_flat_filtered_batch_device";
    leann_backend *h = const_cast<leann_backend *>(hc);
    if (int rc = leann_internal_flat_check_args(who, h, d_queries, nq, top_k, fetch_k, d_keys, d_dists, d_counts)) return rc;
    if (int rc = leann_internal_flat_check_handle(who, h, nq)) return rc;
    if (!d_allow || allow_stride == 0) return leann_backend_search_flat_batch_device(h, d_queries, nq, top_k, fetch_k, d_allow, d_keys, d_dists, d_counts, stream);
    SearchFilter f;
    f.d_allow = d_allow;
    f.allow_stride = allow_stride;
    if (int rc = leann_internal_check_allow_stride(f, h->g.n)) return rc;
    if (nq == 0) return LEANN_OK;
    HIP_CHECK_RET(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t n = h->g.n;
    if (n == 0) {
        HIP_CHECK_RET(hipMemsetAsync(d_counts, 0, nq * 4, st));
        return LEANN_OK;
    }
    const uint8_t *allow = nullptr;
    size_t stride = 0;
    if (int rc = leann_internal_live_allow(h, d_allow, allow_stride, nq, false, st, &allow, &stride)) return rc;
    const size_t per_batch = std::max<size_t>(1, std::min<size_t>(4096, ((size_t)1 << 28) / n));
    for (size_t q0 = 0; q0 < nq; q0 += per_batch) {
        const size_t nb = std::min(per_batch, nq - q0);
        ScratchLease<uint32_t> lists; // both calls below leave the stream synchronised
        std::vector<uint64_t> off;
        if (int rc = leann_internal_compact_allow_batch(allow + q0 * stride, stride, n, nb, &lists, &off, st)) return rc;
        if (int rc = flat_lists_i8_run(h, d_queries + q0 * h->g.d, nb, top_k, fetch_k, off.data(), lists, nullptr, nullptr, d_keys + q0 * top_k,
                                       d_dists + q0 * top_k, d_counts + q0, nullptr, st))
            return rc;
    }
    return LEANN_OK;
}

extern "C" int leann_backend_search_flat_filtered_batch(const leann_backend *h, const float *queries, size_t nq, size_t top_k, size_t fetch_k,
                                                        const uint8_t *allow, size_t allow_stride, uint64_t *keys, float *dists, uint32_t *counts) {
    const char *who = "leann_backend_search_flat_filtered_batch";
    if (int rc = leann_internal_flat_check_args(who, h, queries, nq, top_k, fetch_k, keys, dists, counts)) return rc;
    if (int rc = leann_internal_flat_check_handle(who, h, nq)) return rc;
    if (!allow || allow_stride == 0) return leann_backend_search_flat_batch(h, queries, nq, top_k, fetch_k, allow, keys, dists, counts);
    SearchFilter f;
    f.d_allow = allow; // (only compared with null)
    f.allow_stride = allow_stride;
    if (int rc = leann_internal_check_allow_stride(f, h->g.n)) return rc;
    if (nq == 0) return LEANN_OK;
    if (h->g.n == 0) {
        for (size_t i = 0; i < nq; i++) counts[i] = 0;
        return LEANN_OK;
    }
    HIP_CHECK_RET(hipSetDevice(h->device));
    const size_t d = h->g.d;
    DeviceBuf<float> d_q, d_dists;
    DeviceBuf<uint64_t> d_keys;
    DeviceBuf<uint32_t> d_counts;
    DeviceBuf<uint8_t> d_allow;
    if (int rc = d_q.alloc(nq * d)) return rc;
    if (int rc = d_keys.alloc(nq * top_k)) return rc;
    if (int rc = d_dists.alloc(nq * top_k)) return rc;
    if (int rc = d_counts.alloc(nq)) return rc;
    if (int rc = d_allow.alloc(nq * allow_stride)) return rc;
    HIP_CHECK_RET(hipMemcpy(d_q, queries, nq * d * 4, hipMemcpyHostToDevice));
    HIP_CHECK_RET(hipMemcpy(d_allow, allow, nq * allow_stride, hipMemcpyHostToDevice));
    if (int rc = leann_backend_search_flat_filtered_batch_device(h, d_q, nq, top_k, fetch_k, d_allow, allow_stride, d_keys, d_dists, d_counts, nullptr))
        return rc;
    HIP_CHECK_RET(hipMemcpy(keys, d_keys, nq * top_k * 8, hipMemcpyDeviceToHost));
    HIP_CHECK_RET(hipMemcpy(dists, d_dists, nq * top_k * 4, hipMemcpyDeviceToHost));
    HIP_CHECK_RET(hipMemcpy(counts, d_counts, nq * 4, hipMemcpyDeviceToHost));
    return LEANN_OK;
}
