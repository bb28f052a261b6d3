// scan_i8.hip — exhaustive top-k over int8 rows on the integer matrix cores (include/leann_backend.h "exhaustive search on int8
// rows"): leann_backend_search_flat_batch[_device] and the host reference quantiser leann_quantize_query_i8.
//
// The query gets int8 codes of its own (i8_rows.h: q'_j = q_j 2^-e_j, one power-of-two scale 2^E for the whole query), every row is
// screened by the exact int32 dot product of the two code vectors, the fetch_k best rows by (float)s are scored again with the
// canonical distance of the walk (wave_dist_rows_i8), and the best top_k of those are the answer.  An integer sum does not depend on
// its order, so the store's element permutation (i8_row_pos) is never undone: the query codes are written in store order once, and
// the kernel multiplies store bytes as they lie.
//
// Kernels:
//   quantize_queries_i8_kernel  one wave per query: amax over q' on the DPP ladder, E, the codes written at i8_row_pos(j, ldb) into
//                               Qc [nq rounded up to 64 x ldb] — padding columns and padding queries zero — and one "not finite" word.
//   score_i8_mfma_kernel<LIST>  S[q][i] = (float) sum_j cq[j] c_i[j] with v_mfma_i32_32x32x32_i8; a workgroup of 4 waves owns 128 rows
//                               x 64 queries, wave w the rows 32 w .. 32 w + 31 against all 64 queries (two 32 x 32 i32 tiles).
//                               A = queries, B = rows, as in score_mfma_kernel (scan.hip): a half-wave holds 32 consecutive rows of
//                               one query, so slab stores are 128-B coalesced, and the i32 result layout is the f32 32 x 32 one.
//   rescore_i8_kernel<T>        one workgroup per query; each of its 4 waves takes candidates in turn, the query in registers as the
//                               walk stages it, wave_dist_rows_i8<T, 1> on the candidate's store row; the <= 1 024 keys
//                               orderable(d) << 32 | position are sorted in LDS and the first top_k written.
//
// score_i8_mfma_kernel, data movement.  A k-tile is ONE 128-B line per row (128 codes = four k-steps of the 32-deep MFMA).  Thread t
// loads 16 B of row t / 8 (+ 32 per pass, 4 passes for rows and 2 for queries) at byte 16 (t % 8): a wave instruction reads eight
// whole lines.  The next k-tile travels in registers while the current one is multiplied.  Rows are whole zero-padded lines and Qc
// is padded to the query tile, so there is no tail, no alignment branch and no general form; rows past the end are clamped to the
// launch's last row and their scores are never stored or emitted.  LDS holds sX[128][8] and sQ[64][8] of 16-B columns (24 KiB); the
// line goes in as it is — lane (l31, lh) of k-step s feeds the MFMA column 2 s + lh of its row for BOTH operands, and since any
// assignment of a line's bytes to k positions is right as long as rows and queries share it, nothing is transposed.
//
// Banks.  Column c of row r sits at slot c ^ sw(r), sw(r) = ((r >> 1) & 7) ^ ((r & 1) << 2).  A fragment read is a ds_read_b128 in
// which consecutive lanes read the SAME column of consecutive rows, 128 B apart — unswizzled, every lane would hit the same four
// banks.  Over any aligned 8 consecutive rows sw takes 8 distinct values (the even rows take {a .. a + 3}, the odd ones those ^ 4),
// so 8 lanes cover the 32 four-byte banks of a 128-B line exactly once; over any aligned 16 rows the pairs (r & 1, sw(r)) are all
// distinct, so 16 lanes cover 64 banks (256 B) exactly once: conflict-free whether the LDS serves 128 B or 256 B per clock.  The
// staging write has 8 lanes write the 8 slots of one row (one whole 128-B line) and the next 8 lanes the next row: conflict-free
// for the same reason.  (Reasoned from the layout; the LDS conflict counter was not read.)
//
// Bytes.  Every query tile of grid.y sweeps the rows again: a call reads n ldb ceil(nq / BQ) row bytes, so the wider tile halves the
// row traffic of a batch above 64 queries.  BQ = 64 all the same, by the resource report: at BQ = 128 the 64 accumulators and the
// unrolled epilogue take 199 VGPRs + 64 AGPRs — one wave per SIMD, 47 spilled SGPRs — against 102 + 32 and three waves at BQ = 64.
//
// Resource budget (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; nothing spills, no scratch instruction):
//   quantize_queries_i8_kernel          14 VGPRs,  0 AGPRs, LDS      0 B, 8 waves / SIMD
//   score_i8_mfma_kernel<false | true> 102 VGPRs, 32 AGPRs, LDS 24 576 B, 3 waves / SIMD
//   rescore_i8_kernel<T>, LDS 8 192 B   T = 1: 16 VGPRs, 2: 25, 3: 30, 4: 37, 6: 47 (8 waves / SIMD each), 8: 68 (7), 12: 96 (5), 16: 120 (4)
#include "common.cuh"
#include "../../include/leann_backend.h"
#include "search.cuh"
#include "internal.h"
#include "i8_rows.h"
#include <algorithm>
#include <vector>

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
constexpr uint32_t FLAT_BR = 128, FLAT_BQ = 64; // rows and queries of a workgroup's tile
constexpr size_t FLAT_MAX_K = SEG / 2;           // fetch_k: what leann_scan_topk_device allows for top_k

// ---- the query codes ------------------------------------------------------------------------------------------------------------------
// grid = nq rounded up to FLAT_BQ; scales: g.norms, 2^-e_j [ld >= d].
__global__ void __launch_bounds__(64) quantize_queries_i8_kernel(const float *__restrict__ Q, uint32_t nq, uint32_t d,
                                                                 const float *__restrict__ scales, uint32_t ldb, int8_t *__restrict__ Qc,
                                                                 uint32_t *__restrict__ bad /* [nq] */) {
    const uint32_t q = blockIdx.x, lane = threadIdx.x;
    uint32_t *out = reinterpret_cast<uint32_t *>(Qc + (size_t)q * ldb);
    if (q >= nq) { // a padding query of the last tile
        for (uint32_t g = lane; g < (ldb >> 2); g += 64) out[g] = 0u;
        return;
    }
    const float *qv = Q + (size_t)q * d;
    uint32_t mb = 0; // bits of max |q'_j|: non-negative floats order as their bits do, and a NaN or an infinity is >= 0x7F800000
    for (uint32_t j = lane; j < d; j += 64) mb = max(mb, __float_as_uint(qv[j] * scales[j]) & 0x7FFFFFFFu);
    mb = ~wave_min_u32(~mb);
    const float amax = __uint_as_float(mb);
    const bool finite = i8_query_finite(amax);
    const int E = finite ? i8_query_exponent(amax) : 0;
    // one work item = four elements 4 g .. 4 g + 3 (i8_row_pos keeps groups of four together): every byte of the row is written once
    for (uint32_t g = lane; g < (ldb >> 2); g += 64) {
        const uint32_t j = g << 2;
        uint32_t w = 0;
#pragma unroll
        for (uint32_t e = 0; e < 4; e++)
            if (finite && j + e < d) w |= (uint32_t)(uint8_t)i8_query_code(qv[j + e] * scales[j + e], E) << (8 * e);
        out[i8_row_pos(j, ldb) >> 2] = w;
    }
    if (lane == 0) bad[q] = finite ? 0u : 1u;
}

// ---- the screen -----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t flat_sw(uint32_t r) { return ((r >> 1) & 7u) ^ ((r & 1u) << 2); }

// LIST: row i of the launch is store row idx[row0 + i] (the allowed and live positions, compacted ascending); scores, slab columns and
// emitted keys are then indexed by i, and finalize_scan_kernel (scan.hip) maps i -> idx[i].  Epilogue: score_mfma_kernel's contract.
template <bool LIST>
__global__ void __launch_bounds__(256) score_i8_mfma_kernel(const int8_t *__restrict__ X, uint32_t ldb, const int8_t *__restrict__ Qc,
                                                            uint32_t nq, uint64_t row0, uint32_t n_rows,
                                                            float *__restrict__ S /* [nq x n_rows] */, CandEmit em,
                                                            const uint32_t *__restrict__ idx) {
    constexpr int QT = FLAT_BQ / 32; // 32-query tiles of a wave, and staging passes of the query tile
    __shared__ i32x4 sX[FLAT_BR * 8];
    __shared__ i32x4 sQ[FLAT_BQ * 8];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const uint32_t rbase = blockIdx.x * FLAT_BR, qbase = blockIdx.y * FLAT_BQ;
    i32x16 acc[QT];
#pragma unroll
    for (int t = 0; t < QT; t++)
#pragma unroll
        for (int i = 0; i < 16; i++) acc[t][i] = 0;
    const uint32_t sr = tid >> 3, sc = tid & 7; // staging: row / query sr (+ 32 per pass), 16-B column sc
    const int8_t *xp[4], *qp[QT];
#pragma unroll
    for (int p = 0; p < 4; p++) {
        const uint32_t row = min(rbase + sr + 32 * p, n_rows - 1);
        xp[p] = X + (LIST ? (size_t)idx[row0 + row] : (size_t)(row0 + row)) * ldb + 16 * sc;
    }
#pragma unroll
    for (int p = 0; p < QT; p++) qp[p] = Qc + (size_t)(qbase + sr + 32 * p) * ldb + 16 * sc; // Qc is padded to the tile
    i32x4 xv[4], qv[QT];
    auto gload = [&](uint32_t k0) {
#pragma unroll
        for (int p = 0; p < 4; p++) xv[p] = *reinterpret_cast<const i32x4 *>(xp[p] + k0);
#pragma unroll
        for (int p = 0; p < QT; p++) qv[p] = *reinterpret_cast<const i32x4 *>(qp[p] + k0);
    };
    const uint32_t wslot = sc ^ flat_sw(sr);   // (sw(sr + 32 p) == sw(sr))
    const uint32_t rsw = flat_sw(l31);         // (sw(32 w + l31) == sw(l31))
    gload(0);
    for (uint32_t k0 = 0; k0 < ldb; k0 += 128) {
#pragma unroll
        for (int p = 0; p < 4; p++) sX[(sr + 32 * p) * 8 + wslot] = xv[p];
#pragma unroll
        for (int p = 0; p < QT; p++) sQ[(sr + 32 * p) * 8 + wslot] = qv[p];
        __syncthreads();
        if (k0 + 128 < ldb) gload(k0 + 128);
#pragma unroll
        for (uint32_t s = 0; s < 4; s++) {
            const uint32_t slot = (2 * s + lh) ^ rsw;
            const i32x4 b = sX[(wave * 32 + l31) * 8 + slot];
#pragma unroll
            for (int t = 0; t < QT; t++) acc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(sQ[(32 * t + l31) * 8 + slot], b, acc[t], 0, 0, 0);
        }
        __syncthreads();
    }
    // C/D layout: col = lane & 31 (row of X), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (query).  (float)s: v_cvt_f32_i32, RNE.
    const uint32_t row = rbase + wave * 32 + l31;
    if (em.thr) { // candidate emission (CandEmit, internal.h); a padding query of the last tile (q >= nq) never emits
        bool any = false;
#pragma unroll
        for (int t = 0; t < QT; t++)
#pragma unroll
            for (int reg = 0; reg < 16; reg++) {
                const uint32_t q = qbase + 32 * t + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
                any |= q < nq && (float)acc[t][reg] >= em.thr[q];
            }
        if (any && row < n_rows) {
            const uint64_t pos = em.pos0 + row;
            if (!em.allow || ((em.allow[pos >> 3] >> (pos & 7)) & 1)) {
#pragma unroll
                for (int t = 0; t < QT; t++)
#pragma unroll
                    for (int reg = 0; reg < 16; reg++) {
                        const uint32_t q = qbase + 32 * t + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
                        const float sv = (float)acc[t][reg];
                        if (q < nq && sv >= em.thr[q]) {
                            const uint32_t slot = atomicAdd(&em.cnt[q], 1u);
                            if (slot < em.cap) em.list[(size_t)q * em.cap + slot] = ((uint64_t)(~f32_orderable(sv)) << 32) | (uint32_t)pos;
                        }
                    }
            }
        }
        return;
    }
    if (row < n_rows) {
#pragma unroll
        for (int t = 0; t < QT; t++)
#pragma unroll
            for (int reg = 0; reg < 16; reg++) {
                const uint32_t q = qbase + 32 * t + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
                if (q < nq) S[(size_t)q * n_rows + row] = (float)acc[t][reg];
            }
    }
}

static void launch_score_i8(hipStream_t st, const int8_t *X, uint32_t ldb, const int8_t *Qc, size_t nq, size_t row0, size_t rows, float *S,
                            const CandEmit &em, const uint32_t *idx) {
    const dim3 grid((unsigned)((rows + FLAT_BR - 1) / FLAT_BR), (unsigned)((nq + FLAT_BQ - 1) / FLAT_BQ));
    if (idx) hipLaunchKernelGGL(score_i8_mfma_kernel<true>, grid, dim3(256), 0, st, X, ldb, Qc, (uint32_t)nq, (uint64_t)row0, (uint32_t)rows, S, em, idx);
    else hipLaunchKernelGGL(score_i8_mfma_kernel<false>, grid, dim3(256), 0, st, X, ldb, Qc, (uint32_t)nq, (uint64_t)row0, (uint32_t)rows, S, em, idx);
}

// ---- the answer -----------------------------------------------------------------------------------------------------------------------
struct RescoreArgs {
    const int8_t *X;       // the store, [n x ldb]
    uint64_t n;
    uint32_t ldb, d, ld;
    const float *scales;   // 2^-e_j [ld]
    const float *Q;        // [nq x d]
    const uint64_t *cand;  // [nq x fetch_k] positions, the screen's order
    const uint32_t *cand_cnt, *bad; // [nq]
    uint32_t fetch_k, top_k;
    uint64_t key_offset;
    uint64_t *out_keys;
    float *out_dists;
    uint32_t *out_counts;
};
// The distance is the int8 walk's, bit for bit: the same query staging (beam_search_one, I8) and the same wave_dist_rows_i8<T, 1>.
template <int T>
__global__ void __launch_bounds__(256) rescore_i8_kernel(RescoreArgs a) {
    __shared__ uint64_t keys[FLAT_MAX_K];
    const uint32_t qi = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    const int lane = tid & 63;
    const uint32_t cnt = a.bad[qi] ? 0u : min(a.cand_cnt[qi], a.fetch_k); // a query without codes has no candidates
    int w = 64;
    while (w < (int)cnt) w <<= 1;
    for (uint32_t i = cnt + tid; i < (uint32_t)w; i += 256) keys[i] = ~0ull;
    float4 q[T];
    const float *qv = a.Q + (size_t)qi * a.d;
#pragma unroll
    for (int t = 0; t < T; t++) {
        q[t] = vec_load4_guard(qv, a.d, t, lane);
        const uint32_t j = 256u * t + 4u * lane;
        if (j < a.ld) { // ld is a multiple of 4; the scales of padding columns are 1
            const float4 sc = *reinterpret_cast<const float4 *>(a.scales + j);
            q[t].x *= sc.x; q[t].y *= sc.y; q[t].z *= sc.z; q[t].w *= sc.w;
        }
    }
    for (uint32_t c = wave; c < cnt; c += 4) {
        const uint64_t key = a.cand[(size_t)qi * a.fetch_k + c];
        uint64_t out = ~0ull;
        if (key < a.n) { // checked before an address is formed (the screen only ever lists positions below n)
            const uint32_t ids[1] = {(uint32_t)key};
            float dd[1];
            wave_dist_rows_i8<T, 1>(q, a.X, a.ldb, ids, 1, lane, dd);
            out = ((uint64_t)f32_orderable(dd[0]) << 32) | (uint32_t)key;
        }
        if (lane == 0) keys[c] = out;
    }
    bitonic_sort_lds(keys, w);
    const uint32_t nout = min(cnt, a.top_k);
    for (uint32_t i = tid; i < a.top_k; i += 256) {
        const size_t o = (size_t)qi * a.top_k + i;
        const uint64_t key = i < nout ? keys[i] : ~0ull;
        a.out_keys[o] = i < nout ? (key & 0xFFFFFFFFull) + a.key_offset : ~0ull;
        a.out_dists[o] = i < nout ? orderable_f32((uint32_t)(key >> 32)) : __uint_as_float(0x7F800000u);
    }
    if (tid == 0) a.out_counts[qi] = nout;
}
// the table: one row per row width the int8 walk is compiled for (search_width_T)
using RescoreKernel = void (*)(RescoreArgs);
struct RescoreRow { int T; RescoreKernel kernel; };
template <int T> static constexpr RescoreRow rescore_row() { return {T, rescore_i8_kernel<T>}; }
static RescoreKernel rescore_kernel_of(int T) {
    static constexpr RescoreRow rows[] = {rescore_row<1>(), rescore_row<2>(), rescore_row<3>(), rescore_row<4>(),
                                          rescore_row<6>(), rescore_row<8>(), rescore_row<12>(), rescore_row<16>()};
    for (const RescoreRow &r : rows)
        if (r.T == T) return r.kernel;
    return nullptr;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
// The two ends of a screen over int8 rows (internal.h): the flat search below and the lists search (scan_lists_i8.hip) launch them.
static_assert(FLAT_BQ == 64, "leann_internal_i8_query_rows pads the query codes to the score tile");
int leann_internal_quantize_queries_i8(const leann_backend *h, const float *d_queries, size_t nq, int8_t *Qc, uint32_t *bad, hipStream_t st) {
    const GraphView &g = h->g;
    const uint32_t ldb = g.row_bytes;
    if (!g.X || !g.norms || (ldb & 127u) || ldb < g.ld || !rescore_kernel_of(search_width_T((g.ld + 255) / 256))) {
        leann_set_error("int8 rows: the handle's row store or its column scales are missing or malformed (pitch %u B for %u elements)", ldb, g.ld);
        return LEANN_ERR_INVALID;
    }
    hipLaunchKernelGGL(quantize_queries_i8_kernel, dim3((unsigned)leann_internal_i8_query_rows(nq)), dim3(64), 0, st, d_queries, (uint32_t)nq, g.d,
                       g.norms, ldb, Qc, bad);
    HIP_CHECK_RET(hipGetLastError());
    return LEANN_OK;
}
int leann_internal_rescore_i8(const leann_backend *h, const float *d_queries, size_t nq, const uint64_t *cand, const uint32_t *cand_cnt,
                              const uint32_t *bad, uint32_t fetch_k, uint32_t top_k, uint64_t *d_keys, float *d_dists, uint32_t *d_counts,
                              hipStream_t st) {
    const GraphView &g = h->g;
    const RescoreKernel rescore = rescore_kernel_of(search_width_T((g.ld + 255) / 256));
    if (!rescore) { leann_set_error("int8 rows: no rescore kernel for rows of %u elements", g.ld); return LEANN_ERR_INVALID; }
    RescoreArgs a{};
    a.X = reinterpret_cast<const int8_t *>(g.X); a.n = g.n; a.ldb = g.row_bytes; a.d = g.d; a.ld = g.ld; a.scales = g.norms; a.Q = d_queries;
    a.cand = cand; a.cand_cnt = cand_cnt; a.bad = bad; a.fetch_k = fetch_k; a.top_k = top_k; a.key_offset = h->key_offset;
    a.out_keys = d_keys; a.out_dists = d_dists; a.out_counts = d_counts;
    hipLaunchKernelGGL(rescore, dim3((unsigned)nq), dim3(256), 0, st, a);
    HIP_CHECK_RET(hipGetLastError());
    return LEANN_OK;
}
// The screen follows scan_topk_impl (scan.hip) with k = fetch_k: plan, scratch, begin, per chunk { score, select }, finish, once more on
// the slab schedule if a candidate list overflowed.  Returns with `st` synchronised.
static int flat_i8_run(leann_backend *h, const float *d_queries, size_t nq, size_t top_k, size_t fetch_k, const uint8_t *d_allow,
                       uint64_t *d_keys, float *d_dists, uint32_t *d_counts, hipStream_t st) {
    const GraphView &g = h->g;
    const int8_t *X = reinterpret_cast<const int8_t *>(g.X);
    const uint32_t ldb = g.row_bytes, k = (uint32_t)fetch_k;
    const size_t nq_pad = leann_internal_i8_query_rows(nq);
    // every return, early ones included, gives the scratch back — after the stream is idle (SyncFirst is declared last, so it runs first)
    ScratchLease<int8_t> Qc;
    ScratchLease<uint32_t> bad, candC, list;
    ScratchLease<uint64_t> candK;
    ScratchLease<float> candS;
    struct SyncFirst {
        hipStream_t st;
        ~SyncFirst() { (void)hipStreamSynchronize(st); }
    } sync_first{st};
    if (int e = Qc.acquire(nq_pad * ldb)) return e;
    if (int e = bad.acquire(nq)) return e;
    if (int e = candK.acquire(nq * k)) return e;
    if (int e = candS.acquire(nq * k)) return e;
    if (int e = candC.acquire(nq)) return e;
    if (int rc = leann_internal_quantize_queries_i8(h, d_queries, nq, Qc, bad, st)) return rc;
    // the rows of the screen: all of them, or the allowed AND live ones as an ascending list
    const uint8_t *allow = nullptr;
    size_t allow_stride = 0, m = g.n;
    if (int rc = leann_internal_live_allow(h, d_allow, 0, nq, false, st, &allow, &allow_stride)) return rc;
    if (allow)
        if (int rc = leann_internal_compact_allow(allow, g.n, &list, &m, st)) return rc;
    const uint32_t *idx = allow ? list.p : nullptr;
    if (m == 0) HIP_CHECK_RET(hipMemsetAsync(candC, 0, nq * 4, st)); // nothing to screen: the rescore kernel writes the empty answers
    const TopkShape shape = topk_shape_scan(m, nq, k);
    for (bool emit = m > shape.emit_first && !leann_knobs().no_emit; m != 0; emit = false) {
        TopkRun run{topk_plan(shape, emit)};
        const TopkPlan &p = run.plan;
        ScratchLease<float> S;
        ScratchLease<uint64_t> candA, candB, best;
        ScratchLease<unsigned char> emb;
        SyncFirst sync_pass{st};
        if (int e = S.acquire(shape.q_tile * p.slab_rows)) return e;
        if (int e = candA.acquire(nq * p.cand_len)) return e;
        if (int e = candB.acquire(nq * p.cand_len)) return e;
        if (int e = best.acquire(nq * k)) return e;
        if (p.emit)
            if (int e = emb.acquire(p.emit_bytes)) return e;
        run.S = S, run.candA = candA, run.candB = candB, run.best = best, run.emit_block = emb;
        run.nq = nq, run.k = k, run.allow = nullptr, run.st = st;
        int rc = leann_internal_topk_begin(run);
        for (size_t c = 0; c < p.chunks.size() && rc == LEANN_OK; c++) {
            launch_score_i8(st, X, ldb, Qc, nq, p.chunks[c].first, p.chunks[c].second, S, run.chunk_emit(c), idx);
            rc = leann_internal_topk_select_chunk(run, c, 0, (uint32_t)nq);
        }
        bool overflowed = false;
        // keys = positions (idx maps list entries back), no key offset yet; the screen's scores are not part of the answer
        if (rc == LEANN_OK) rc = leann_internal_topk_finish(run, 0, idx, 0, candK, candS, candC, &overflowed);
        if (rc != LEANN_OK) return rc;
        if (!overflowed) break;
    }
    if (int rc = leann_internal_rescore_i8(h, d_queries, nq, candK, candC, bad, k, (uint32_t)top_k, d_keys, d_dists, d_counts, st)) return rc;
    HIP_CHECK_RET(hipStreamSynchronize(st));
    return LEANN_OK;
}

// what the entry points refuse, on the host, before any device work (internal.h; the lists search of scan_lists_i8.hip refuses the
// same): null arguments, then k out of range (the handle is not read before these), then the handles the screen is not defined for
int leann_internal_flat_check_args(const char *who, const leann_backend *h, const void *queries, size_t nq, size_t top_k, size_t fetch_k,
                                   const void *keys, const void *dists, const void *counts) {
    if (!h || (nq && (!queries || !keys || !dists || !counts))) {
        leann_set_error("%s: null %s", who, !h ? "handle" : !queries ? "queries" : !keys ? "keys" : !dists ? "dists" : "counts");
        return LEANN_ERR_INVALID;
    }
    if (top_k == 0) { leann_set_error("%s: top_k = 0", who); return LEANN_ERR_INVALID; }
    if (fetch_k > FLAT_MAX_K) { leann_set_error("%s: fetch_k = %zu is above %zu", who, fetch_k, FLAT_MAX_K); return LEANN_ERR_INVALID; }
    if (top_k > fetch_k) { leann_set_error("%s: top_k = %zu is above fetch_k = %zu", who, top_k, fetch_k); return LEANN_ERR_INVALID; }
    return LEANN_OK;
}
int leann_internal_flat_check_handle(const char *who, const leann_backend *h, size_t nq) {
    if (h->sharded) {
        leann_set_error("%s is not available on a composite handle (search each shard with leann_backend_shard(h, g) and merge with leann_merge_topk_device)", who);
        return LEANN_ERR_UNSUPPORTED;
    }
    if (h->g.feat_h) {
        leann_set_error("%s needs stored int8 rows; this index recomputes its vectors from features (use leann_recompute_search_batch_device)", who);
        return LEANN_ERR_UNSUPPORTED;
    }
    if (h->row_type == LEANN_ROWS_F32) {
        leann_set_error("%s screens int8 rows; this index stores f32 rows (use leann_backend_search_filtered_exact_batch, or leann_scan_topk_device "
                        "over leann_backend_device_rows)", who);
        return LEANN_ERR_UNSUPPORTED;
    }
    if (!leann_internal_i8(h)) {
        leann_set_error("%s screens int8 rows; this index stores %s rows, whose screen would have to round the query (use the walk, or "
                        "leann_backend_search_refined_batch)", who, leann_internal_row_name(h));
        return LEANN_ERR_UNSUPPORTED;
    }
    if (h->g.n >= (1ull << 32) || nq >= (1ull << 31)) {
        leann_set_error("%s: the index has 2^32 rows or more, or nq = %zu is 2^31 or more", who, nq);
        return LEANN_ERR_INVALID;
    }
    return LEANN_OK;
}
static int flat_check(const char *who, const leann_backend *h, const void *queries, size_t nq, size_t top_k, size_t fetch_k, const void *keys,
                      const void *dists, const void *counts) {
    if (int rc = leann_internal_flat_check_args(who, h, queries, nq, top_k, fetch_k, keys, dists, counts)) return rc;
    return leann_internal_flat_check_handle(who, h, nq);
}

extern "C" int leann_backend_search_flat_batch_device(const leann_backend *hc, const float *d_queries, size_t nq, size_t top_k, size_t fetch_k,
                                                      const uint8_t *d_allow, uint64_t *d_keys, float *d_dists, uint32_t *d_counts, void *stream) {
    leann_backend *h = const_cast<leann_backend *>(hc);
    if (int rc = flat_check("leann_backend_search_flat_batch_device", h, d_queries, nq, top_k, fetch_k, d_keys, d_dists, d_counts)) return rc;
    if (nq == 0) return LEANN_OK;
    HIP_CHECK_RET(hipSetDevice(h->device));
    if (h->g.n == 0) {
        HIP_CHECK_RET(hipMemsetAsync(d_counts, 0, nq * 4, (hipStream_t)stream));
        return LEANN_OK;
    }
    return flat_i8_run(h, d_queries, nq, top_k, fetch_k, d_allow, d_keys, d_dists, d_counts, (hipStream_t)stream);
}

extern "C" int leann_backend_search_flat_batch(const leann_backend *hc, const float *queries, size_t nq, size_t top_k, size_t fetch_k,
                                               const uint8_t *allow, uint64_t *keys, float *dists, uint32_t *counts) {
    leann_backend *h = const_cast<leann_backend *>(hc);
    if (int rc = flat_check("leann_backend_search_flat_batch", h, queries, nq, top_k, fetch_k, keys, dists, counts)) return rc;
    if (nq == 0) return LEANN_OK;
    if (h->g.n == 0) { // nothing to search: answered on the host
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
    HIP_CHECK_RET(hipMemcpy(d_q, queries, nq * d * 4, hipMemcpyHostToDevice));
    if (allow) {
        if (int rc = d_allow.alloc((h->g.n + 7) / 8)) return rc;
        HIP_CHECK_RET(hipMemcpy(d_allow, allow, (h->g.n + 7) / 8, hipMemcpyHostToDevice));
    }
    if (int rc = flat_i8_run(h, d_q, nq, top_k, fetch_k, allow ? d_allow.p : nullptr, d_keys, d_dists, d_counts, nullptr)) return rc;
    HIP_CHECK_RET(hipMemcpy(keys, d_keys, nq * top_k * 8, hipMemcpyDeviceToHost));
    HIP_CHECK_RET(hipMemcpy(dists, d_dists, nq * top_k * 4, hipMemcpyDeviceToHost));
    HIP_CHECK_RET(hipMemcpy(counts, d_counts, nq * 4, hipMemcpyDeviceToHost));
    return LEANN_OK;
}

// the reference the device quantiser is held to: i8_rows.h's arithmetic, element order, no device
extern "C" int leann_quantize_query_i8(const float *q, size_t d, const int8_t *exps, int8_t *codes_out, int32_t *E_out) {
    if (!q || !exps || !codes_out || !E_out || d == 0) {
        leann_set_error("leann_quantize_query_i8: null %s", !q ? "q" : !exps ? "exps" : !codes_out ? "codes_out" : !E_out ? "E_out" : "query (d = 0)");
        return LEANN_ERR_INVALID;
    }
    uint32_t mb = 0;
    for (size_t j = 0; j < d; j++) {
        const float qs = q[j] * i8_pow2(-exps[j]);
        uint32_t b;
        memcpy(&b, &qs, 4);
        mb = std::max(mb, b & 0x7FFFFFFFu);
    }
    float amax;
    memcpy(&amax, &mb, 4);
    const bool finite = i8_query_finite(amax);
    const int E = finite ? i8_query_exponent(amax) : 0;
    for (size_t j = 0; j < d; j++) codes_out[j] = finite ? i8_query_code(q[j] * i8_pow2(-exps[j]), E) : (int8_t)0;
    *E_out = finite ? E : LEANN_I8_QUERY_NONFINITE;
    return LEANN_OK;
}
