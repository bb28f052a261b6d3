// scan_bf16.hip — exhaustive top-k over bf16 rows on the bf16 matrix cores (include/leann_backend.h "exhaustive search on bf16
// rows"): leann_backend_search_flat_bf16_batch[_device] and the host reference split leann_split_query_bf16.
//
// The query is NOT rounded: it is split into two bf16 pieces, hi_j = r(q_j) and lo_j = r(q_j - w(hi_j)) (r, w: bf16.h; the
// subtraction is exact), so w(hi_j) + w(lo_j) is q_j to within 2^-17 |q_j|.  Every row is screened by
//     s_i = sum_j (w(hi_j) + w(lo_j)) w(x_ij)
// — each product of two bf16 values is exact in f32; the sum is accumulated in f32 by v_mfma_f32_32x32x16_bf16 in an order the
// definition leaves open —, the fetch_k best rows by s are scored again with the canonical distance of the bf16 walk
// (wave_dist_rows_bf16), and the best top_k of those are the answer.  A sum that is order-free up to rounding lets the store's
// element permutation (rs_plane_pos) stand: the query pieces are written in store order once, and the kernel multiplies store
// halves as they lie.
//
// Kernels:
//   split_queries_bf16_kernel     one wave per query: the two pieces written at rs_plane_pos(j, ldb) into Qhi and Qlo
//                                 [nq rounded up to FLAT16_BQ x ldb] u16 — padding columns and padding queries zero — and one "not
//                                 finite" word (some w(hi_j) is not finite: the pieces are then written as zeros).
//   score_bf16_mfma_kernel<LIST>  S[q][i] = s_i of query q; a workgroup of 4 waves owns 128 rows x FLAT16_BQ queries, wave w the rows
//                                 32 w .. 32 w + 31 against all queries of the tile.  A = query pieces, B = rows, as in
//                                 score_mfma_kernel (scan.hip): the f32 32 x 32 result layout, so its epilogue contract (slab S, or
//                                 CandEmit against em.thr) and everything behind it is reused unchanged.  Per k-step two MFMAs per
//                                 32-query tile, hi then lo, into the same accumulator.
//   rescore_bf16_kernel<T>        one workgroup per query; each of its 4 waves takes candidates in turn, the query in registers as the
//                                 walk stages it, wave_dist_rows_bf16<T, 1> on the candidate's store row; the <= 1 024 keys
//                                 orderable(d) << 32 | position are sorted in LDS and the first top_k written.
//
// score_bf16_mfma_kernel, data movement.  A k-tile is ONE 128-B line per row: 64 bf16 elements = four k-steps of the 16-deep MFMA,
// whose operand is 8 bf16 = 16 B per lane.  Thread t loads 16 B of row t / 8 (+ 32 per pass: 4 passes for rows, FLAT16_BQ / 32 for
// each of Qhi and Qlo) at byte 16 (t % 8): a wave instruction reads eight whole lines.  The next k-tile travels in registers while
// the current one is multiplied.  Rows are whole zero-padded lines and the pieces are padded to the query tile, so there is no tail,
// no alignment branch and no general form; rows past the end are clamped to the launch's last row and their scores are never
// stored or emitted.  LDS holds sX[128][8], sQhi[BQ][8] and sQlo[BQ][8] of 16-B columns.  The line goes in as it lies: lane
// (l31, lh) of k-step s feeds the MFMA the 16-B column 2 s + lh of its row for BOTH operands (k = 8 lh .. 8 lh + 7 of the step),
// and since any assignment of a line's elements to k positions is right as long as rows and pieces share it, nothing is transposed.
//
// Banks, for this operand width.  An operand of 8 bf16 is 16 B, so a 128-B line is 8 columns of 16 B and a fragment read is a
// ds_read_b128: the geometry the int8 kernel (scan_i8.hip) has with 16 codes per lane, and its argument carries over column for
// column.  Column c of row r sits at slot c ^ sw(r), sw(r) = ((r >> 1) & 7) ^ ((r & 1) << 2).  In a fragment read consecutive
// lanes read the SAME column of consecutive rows, 128 B apart — unswizzled, every lane would hit the same four banks.  Over any
// aligned 8 consecutive rows sw takes 8 distinct values (the even rows take {a .. a + 3}, the odd ones those ^ 4), so 8 lanes
// cover the 32 four-byte banks of a 128-B line exactly once; over any aligned 16 rows the pairs (r & 1, sw(r)) are all distinct,
// so 16 lanes cover 64 banks (256 B) exactly once: conflict-free whether the LDS serves 128 B or 256 B per clock.  The staging
// write has 8 lanes write the 8 slots of one row (one whole 128-B line) and the next 8 lanes the next row: conflict-free for the
// same reason.  (Reasoned from the layout; the LDS conflict counter was not read.)
//
// Bytes and the query tile.  Every query tile of grid.y sweeps the rows again: a call reads n pitch ceil(nq / BQ) row bytes, so the
// wider tile would halve the row traffic of a batch above 64 queries.  BQ = 64 all the same, by the resource report: at BQ = 128
// (-DLEANN_FLAT16_BQ=128) the 64 accumulators, the 12 staged 16-B columns and the unrolled epilogue take 199 VGPRs + 64 AGPRs — one
// wave per SIMD, 47 spilled SGPRs, LDS 49 152 B — against 102 + 32 and three waves at BQ = 64.
//
// Resource budget (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; nothing spills, no scratch instruction):
//   split_queries_bf16_kernel            18 VGPRs,  0 AGPRs, LDS      0 B, 8 waves / SIMD
//   score_bf16_mfma_kernel<false | true> 102 VGPRs, 32 AGPRs, LDS 32 768 B, 3 waves / SIMD
//   rescore_bf16_kernel<T>, LDS 8 192 B   T = 1: 15 VGPRs, 2: 26, 3: 30, 4: 36, 6: 48, 8: 60 (8 waves / SIMD each), 12: 92 (5), 16: 124 (4)
#include "common.cuh"
#include "../../include/leann_backend.h"
#include "search.cuh"
#include "internal.h"
#include "bf16.h"
#include "row_screen.h"
#include <algorithm>

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
#ifndef LEANN_FLAT16_BQ
#define LEANN_FLAT16_BQ 64
#endif
constexpr uint32_t FLAT16_BR = 128, FLAT16_BQ = LEANN_FLAT16_BQ; // rows and queries of a workgroup's tile
constexpr size_t FLAT16_MAX_K = SEG / 2;                          // fetch_k: what leann_scan_topk_device allows for top_k
static_assert(FLAT16_BQ == 64 || FLAT16_BQ == 128, "the query tile is two or four 32-query MFMA tiles");

static size_t query_rows(size_t nq) { return (nq + FLAT16_BQ - 1) / FLAT16_BQ * FLAT16_BQ; }

// ---- the query pieces -----------------------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ bool bf16_finite(uint16_t b) { return (b & 0x7F80u) != 0x7F80u; }
__host__ __device__ __forceinline__ float bf16_widen(uint16_t b) {
    const uint32_t u = (uint32_t)b << 16;
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float f;
    memcpy(&f, &u, 4);
    return f;
#endif
}
__host__ __device__ __forceinline__ uint16_t split_lo(float q, uint16_t hi) { return f32_to_bf16_rne(q - bf16_widen(hi)); }

// grid = nq rounded up to FLAT16_BQ.  ldb: elements of a store row (a multiple of 64).
__global__ void __launch_bounds__(64) split_queries_bf16_kernel(const float *__restrict__ Q, uint32_t nq, uint32_t d, uint32_t ldb,
                                                                uint16_t *__restrict__ Qhi, uint16_t *__restrict__ Qlo,
                                                                uint32_t *__restrict__ bad /* [nq] */) {
    const uint32_t q = blockIdx.x, lane = threadIdx.x;
    uint16_t *ohi = Qhi + (size_t)q * ldb, *olo = Qlo + (size_t)q * ldb;
    const float *qv = Q + (size_t)q * d;
    uint32_t nonfinite = 0;
    if (q < nq)
        for (uint32_t j = lane; j < d; j += 64) nonfinite |= bf16_finite(f32_to_bf16_rne(qv[j])) ? 0u : 1u;
    const bool finite = q < nq && wave_min_u32(nonfinite ^ 1u) != 0u; // (a padding query of the last tile: zero pieces)
    // one work item = four elements 4 g .. 4 g + 3 (rs_plane_pos keeps groups of four together): every half of both rows is written once
    for (uint32_t g = lane; g < (ldb >> 2); g += 64) {
        const uint32_t j = g << 2;
        uint16_t hi[4] = {0, 0, 0, 0}, lo[4] = {0, 0, 0, 0};
#pragma unroll
        for (uint32_t e = 0; e < 4; e++)
            if (finite && j + e < d) {
                hi[e] = f32_to_bf16_rne(qv[j + e]);
                lo[e] = split_lo(qv[j + e], hi[e]);
            }
        const uint32_t pos = rs_plane_pos(j, ldb);
        *reinterpret_cast<uint2 *>(ohi + pos) = make_uint2((uint32_t)hi[0] | ((uint32_t)hi[1] << 16), (uint32_t)hi[2] | ((uint32_t)hi[3] << 16));
        *reinterpret_cast<uint2 *>(olo + pos) = make_uint2((uint32_t)lo[0] | ((uint32_t)lo[1] << 16), (uint32_t)lo[2] | ((uint32_t)lo[3] << 16));
    }
    if (lane == 0 && q < nq) bad[q] = finite ? 0u : 1u;
}

// ---- the screen -----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t flat16_sw(uint32_t r) { return ((r >> 1) & 7u) ^ ((r & 1u) << 2); }

// X: the store, n rows `pitch` bytes apart.  LIST: row i of the launch is store row idx[row0 + i] (the allowed and live positions,
// compacted ascending); scores, slab columns and emitted keys are then indexed by i, and finalize_scan_kernel (scan.hip) maps
// i -> idx[i].  A position is compared with n before it becomes an address (a list entry at or beyond n reads row n - 1; its score
// is one of a row that exists).  Epilogue: score_mfma_kernel's contract.
template <bool LIST>
__global__ void __launch_bounds__(256) score_bf16_mfma_kernel(const unsigned char *__restrict__ X, uint64_t n, uint32_t pitch,
                                                              const unsigned char *__restrict__ Qhi, const unsigned char *__restrict__ Qlo,
                                                              uint32_t nq, uint64_t row0, uint32_t n_rows,
                                                              float *__restrict__ S /* [nq x n_rows] */, CandEmit em,
                                                              const uint32_t *__restrict__ idx) {
    constexpr int QT = FLAT16_BQ / 32; // 32-query tiles of a wave, and staging passes of each piece tile
    __shared__ i32x4 sX[FLAT16_BR * 8];
    __shared__ i32x4 sQhi[FLAT16_BQ * 8];
    __shared__ i32x4 sQlo[FLAT16_BQ * 8];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const uint32_t rbase = blockIdx.x * FLAT16_BR, qbase = blockIdx.y * FLAT16_BQ;
    f32x16 acc[QT];
#pragma unroll
    for (int t = 0; t < QT; t++)
#pragma unroll
        for (int i = 0; i < 16; i++) acc[t][i] = 0.f;
    const uint32_t sr = tid >> 3, sc = tid & 7; // staging: row / query sr (+ 32 per pass), 16-B column sc
    const unsigned char *xp[4], *hp[QT], *lp[QT];
#pragma unroll
    for (int p = 0; p < 4; p++) {
        const uint32_t row = min(rbase + sr + 32 * p, n_rows - 1);
        const uint64_t pos = LIST ? (uint64_t)idx[row0 + row] : row0 + row;
        xp[p] = X + (size_t)min(pos, n - 1) * pitch + 16 * sc;
    }
#pragma unroll
    for (int p = 0; p < QT; p++) { // the pieces are padded to the tile
        hp[p] = Qhi + (size_t)(qbase + sr + 32 * p) * pitch + 16 * sc;
        lp[p] = Qlo + (size_t)(qbase + sr + 32 * p) * pitch + 16 * sc;
    }
    i32x4 xv[4], hv[QT], lv[QT];
    auto gload = [&](uint32_t k0) {
#pragma unroll
        for (int p = 0; p < 4; p++) xv[p] = *reinterpret_cast<const i32x4 *>(xp[p] + k0);
#pragma unroll
        for (int p = 0; p < QT; p++) {
            hv[p] = *reinterpret_cast<const i32x4 *>(hp[p] + k0);
            lv[p] = *reinterpret_cast<const i32x4 *>(lp[p] + k0);
        }
    };
    const uint32_t wslot = sc ^ flat16_sw(sr); // (sw(sr + 32 p) == sw(sr))
    const uint32_t rsw = flat16_sw(l31);       // (sw(32 w + l31) == sw(l31))
    gload(0);
    for (uint32_t k0 = 0; k0 < pitch; k0 += 128) {
#pragma unroll
        for (int p = 0; p < 4; p++) sX[(sr + 32 * p) * 8 + wslot] = xv[p];
#pragma unroll
        for (int p = 0; p < QT; p++) {
            sQhi[(sr + 32 * p) * 8 + wslot] = hv[p];
            sQlo[(sr + 32 * p) * 8 + wslot] = lv[p];
        }
        __syncthreads();
        if (k0 + 128 < pitch) gload(k0 + 128);
#pragma unroll
        for (uint32_t s = 0; s < 4; s++) {
            const uint32_t slot = (2 * s + lh) ^ rsw;
            const bf16x8 b = __builtin_bit_cast(bf16x8, sX[(wave * 32 + l31) * 8 + slot]);
#pragma unroll
            for (int t = 0; t < QT; t++) {
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, sQhi[(32 * t + l31) * 8 + slot]), b, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, sQlo[(32 * t + l31) * 8 + slot]), b, acc[t], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // C/D layout: col = lane & 31 (row of X), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (query)
    const uint32_t row = rbase + wave * 32 + l31;
    if (em.thr) { // candidate emission (CandEmit, internal.h); a padding query of the last tile (q >= nq) never emits
        bool any = false;
#pragma unroll
        for (int t = 0; t < QT; t++)
#pragma unroll
            for (int reg = 0; reg < 16; reg++) {
                const uint32_t q = qbase + 32 * t + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
                any |= q < nq && acc[t][reg] >= em.thr[q];
            }
        if (any && row < n_rows) {
            const uint64_t pos = em.pos0 + row;
            if (!em.allow || ((em.allow[pos >> 3] >> (pos & 7)) & 1)) {
#pragma unroll
                for (int t = 0; t < QT; t++)
#pragma unroll
                    for (int reg = 0; reg < 16; reg++) {
                        const uint32_t q = qbase + 32 * t + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
                        const float sv = acc[t][reg];
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
                if (q < nq) S[(size_t)q * n_rows + row] = acc[t][reg];
            }
    }
}

static void launch_score_bf16(hipStream_t st, const GraphView &g, const uint16_t *Qhi, const uint16_t *Qlo, size_t nq, size_t row0, size_t rows,
                              float *S, const CandEmit &em, const uint32_t *idx) {
    const dim3 grid((unsigned)((rows + FLAT16_BR - 1) / FLAT16_BR), (unsigned)((nq + FLAT16_BQ - 1) / FLAT16_BQ));
    const unsigned char *X = reinterpret_cast<const unsigned char *>(g.X), *hi = reinterpret_cast<const unsigned char *>(Qhi),
                        *lo = reinterpret_cast<const unsigned char *>(Qlo);
    if (idx) hipLaunchKernelGGL(score_bf16_mfma_kernel<true>, grid, dim3(256), 0, st, X, g.n, g.row_bytes, hi, lo, (uint32_t)nq, (uint64_t)row0, (uint32_t)rows, S, em, idx);
    else hipLaunchKernelGGL(score_bf16_mfma_kernel<false>, grid, dim3(256), 0, st, X, g.n, g.row_bytes, hi, lo, (uint32_t)nq, (uint64_t)row0, (uint32_t)rows, S, em, idx);
}

// ---- the answer -----------------------------------------------------------------------------------------------------------------------
struct Rescore16Args {
    const uint16_t *X;     // the store, [n x ldb] u16
    uint64_t n;
    uint32_t ldb, d;
    const float *Q;        // [nq x d]
    const uint64_t *cand;  // [nq x fetch_k] positions, the screen's order
    const uint32_t *cand_cnt, *bad; // [nq]
    uint32_t fetch_k, top_k;
    uint64_t key_offset;
    uint64_t *out_keys;
    float *out_dists;
    uint32_t *out_counts;
};
// The distance is the bf16 walk's, bit for bit: the same query staging (beam_search_one, BF16) and the same wave_dist_rows_bf16<T, 1>.
template <int T>
__global__ void __launch_bounds__(256) rescore_bf16_kernel(Rescore16Args a) {
    __shared__ uint64_t keys[FLAT16_MAX_K];
    const uint32_t qi = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    const int lane = tid & 63;
    const uint32_t cnt = a.bad[qi] ? 0u : min(a.cand_cnt[qi], a.fetch_k); // a query without pieces has no candidates
    int w = 64;
    while (w < (int)cnt) w <<= 1;
    for (uint32_t i = cnt + tid; i < (uint32_t)w; i += 256) keys[i] = ~0ull;
    float4 q[T];
    const float *qv = a.Q + (size_t)qi * a.d;
#pragma unroll
    for (int t = 0; t < T; t++) q[t] = vec_load4_guard(qv, a.d, t, lane);
    for (uint32_t c = wave; c < cnt; c += 4) {
        const uint64_t key = a.cand[(size_t)qi * a.fetch_k + c];
        uint64_t out = ~0ull;
        if (key < a.n) { // checked before an address is formed (the screen only ever lists positions below n)
            const uint32_t ids[1] = {(uint32_t)key};
            float dd[1];
            wave_dist_rows_bf16<T, 1>(q, a.X, a.ldb, ids, 1, lane, dd);
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
// the table: one row per row width the bf16 walk is compiled for (search_width_T)
using Rescore16Kernel = void (*)(Rescore16Args);
struct Rescore16Row { int T; Rescore16Kernel kernel; };
template <int T> static constexpr Rescore16Row rescore16_row() { return {T, rescore_bf16_kernel<T>}; }
static Rescore16Kernel rescore16_kernel_of(int T) {
    static constexpr Rescore16Row rows[] = {rescore16_row<1>(), rescore16_row<2>(), rescore16_row<3>(), rescore16_row<4>(),
                                            rescore16_row<6>(), rescore16_row<8>(), rescore16_row<12>(), rescore16_row<16>()};
    for (const Rescore16Row &r : rows)
        if (r.T == T) return r.kernel;
    return nullptr;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
// The screen follows flat_i8_run (scan_i8.hip) and through it scan_topk_impl (scan.hip) with k = fetch_k: plan, scratch, begin, per
// chunk { score, select }, finish, once more on the slab schedule if a candidate list overflowed.  Returns with `st` synchronised.
static int flat_bf16_run(leann_backend *h, const float *d_queries, size_t nq, size_t top_k, size_t fetch_k, const uint8_t *d_allow,
                         uint64_t *d_keys, float *d_dists, uint32_t *d_counts, hipStream_t st) {
    const GraphView &g = h->g;
    const uint32_t ldb = g.row_bytes >> 1, k = (uint32_t)fetch_k;
    const Rescore16Kernel rescore = rescore16_kernel_of(search_width_T((g.ld + 255) / 256));
    if (!g.X || (g.row_bytes & 127u) || ldb < g.ld || !rescore) {
        leann_set_error("bf16 rows: the handle's row store is missing or malformed (pitch %u B for %u elements)", g.row_bytes, g.ld);
        return LEANN_ERR_INVALID;
    }
    const size_t nq_pad = query_rows(nq);
    // every return, early ones included, gives the scratch back — after the stream is idle (SyncFirst is declared last, so it runs first)
    ScratchLease<uint16_t> Qhi, Qlo;
    ScratchLease<uint32_t> bad, candC, list;
    ScratchLease<uint64_t> candK;
    ScratchLease<float> candS;
    struct SyncFirst {
        hipStream_t st;
        ~SyncFirst() { (void)hipStreamSynchronize(st); }
    } sync_first{st};
    if (int e = Qhi.acquire(nq_pad * ldb)) return e;
    if (int e = Qlo.acquire(nq_pad * ldb)) return e;
    if (int e = bad.acquire(nq)) return e;
    if (int e = candK.acquire(nq * k)) return e;
    if (int e = candS.acquire(nq * k)) return e;
    if (int e = candC.acquire(nq)) return e;
    hipLaunchKernelGGL(split_queries_bf16_kernel, dim3((unsigned)nq_pad), dim3(64), 0, st, d_queries, (uint32_t)nq, g.d, ldb, Qhi.p, Qlo.p, bad.p);
    HIP_CHECK_RET(hipGetLastError());
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
            launch_score_bf16(st, g, Qhi, Qlo, nq, p.chunks[c].first, p.chunks[c].second, S, run.chunk_emit(c), idx);
            rc = leann_internal_topk_select_chunk(run, c, 0, (uint32_t)nq);
        }
        bool overflowed = false;
        // keys = positions (idx maps list entries back), no key offset yet; the screen's scores are not part of the answer
        if (rc == LEANN_OK) rc = leann_internal_topk_finish(run, 0, idx, 0, candK, candS, candC, &overflowed);
        if (rc != LEANN_OK) return rc;
        if (!overflowed) break;
    }
    Rescore16Args a{};
    a.X = reinterpret_cast<const uint16_t *>(g.X); a.n = g.n; a.ldb = ldb; a.d = g.d; a.Q = d_queries;
    a.cand = candK; a.cand_cnt = candC; a.bad = bad; a.fetch_k = k; a.top_k = (uint32_t)top_k; a.key_offset = h->key_offset;
    a.out_keys = d_keys; a.out_dists = d_dists; a.out_counts = d_counts;
    hipLaunchKernelGGL(rescore, dim3((unsigned)nq), dim3(256), 0, st, a);
    HIP_CHECK_RET(hipGetLastError());
    HIP_CHECK_RET(hipStreamSynchronize(st));
    return LEANN_OK;
}

// what the entry points refuse, on the host, before any device work: null arguments and k out of range (the handle is not read
// before these: leann_internal_flat_check_args, scan_i8.hip), then the handles the screen is not defined for
static int flat16_check(const char *who, const leann_backend *h, const void *queries, size_t nq, size_t top_k, size_t fetch_k, const void *keys,
                        const void *dists, const void *counts) {
    if (int rc = leann_internal_flat_check_args(who, h, queries, nq, top_k, fetch_k, keys, dists, counts)) return rc;
    if (h->sharded) {
        leann_set_error("%s is not available on a composite handle (search each shard with leann_backend_shard(h, g) and merge with leann_merge_topk_device)", who);
        return LEANN_ERR_UNSUPPORTED;
    }
    if (h->g.feat_h) {
        leann_set_error("%s needs stored bf16 rows; this index recomputes its vectors from features (use leann_recompute_search_batch_device)", who);
        return LEANN_ERR_UNSUPPORTED;
    }
    if (h->row_type == LEANN_ROWS_F32) {
        leann_set_error("%s screens bf16 rows; this index stores f32 rows (use leann_backend_search_filtered_exact_batch, or leann_scan_topk_device "
                        "over leann_backend_device_rows)", who);
        return LEANN_ERR_UNSUPPORTED;
    }
    if (!leann_internal_bf16(h)) {
        leann_set_error("%s screens bf16 rows; this index stores %s rows (use leann_backend_search_flat_batch)", who, leann_internal_row_name(h));
        return LEANN_ERR_UNSUPPORTED;
    }
    if (h->g.n >= (1ull << 32) || nq >= (1ull << 31)) {
        leann_set_error("%s: the index has 2^32 rows or more, or nq = %zu is 2^31 or more", who, nq);
        return LEANN_ERR_INVALID;
    }
    return LEANN_OK;
}

extern "C" int leann_backend_search_flat_bf16_batch_device(const leann_backend *hc, const float *d_queries, size_t nq, size_t top_k,
                                                           size_t fetch_k, const uint8_t *d_allow, uint64_t *d_keys, float *d_dists,
                                                           uint32_t *d_counts, void *stream) {
    leann_backend *h = const_cast<leann_backend *>(hc);
    if (int rc = flat16_check("leann_backend_search_flat_bf16_batch_device", h, d_queries, nq, top_k, fetch_k, d_keys, d_dists, d_counts)) return rc;
    if (nq == 0) return LEANN_OK;
    HIP_CHECK_RET(hipSetDevice(h->device));
    if (h->g.n == 0) {
        HIP_CHECK_RET(hipMemsetAsync(d_counts, 0, nq * 4, (hipStream_t)stream));
        return LEANN_OK;
    }
    return flat_bf16_run(h, d_queries, nq, top_k, fetch_k, d_allow, d_keys, d_dists, d_counts, (hipStream_t)stream);
}

extern "C" int leann_backend_search_flat_bf16_batch(const leann_backend *hc, const float *queries, size_t nq, size_t top_k, size_t fetch_k,
                                                    const uint8_t *allow, uint64_t *keys, float *dists, uint32_t *counts) {
    leann_backend *h = const_cast<leann_backend *>(hc);
    if (int rc = flat16_check("leann_backend_search_flat_bf16_batch", h, queries, nq, top_k, fetch_k, keys, dists, counts)) return rc;
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
    if (int rc = flat_bf16_run(h, d_q, nq, top_k, fetch_k, allow ? d_allow.p : nullptr, d_keys, d_dists, d_counts, nullptr)) return rc;
    HIP_CHECK_RET(hipMemcpy(keys, d_keys, nq * top_k * 8, hipMemcpyDeviceToHost));
    HIP_CHECK_RET(hipMemcpy(dists, d_dists, nq * top_k * 4, hipMemcpyDeviceToHost));
    HIP_CHECK_RET(hipMemcpy(counts, d_counts, nq * 4, hipMemcpyDeviceToHost));
    return LEANN_OK;
}

// the reference the device split is held to: bf16.h's rounding, element order, no device.  The pieces are written element by
// element whatever the query holds; whether the query HAS pieces (every w(hi_j) finite) is the search's decision.
extern "C" int leann_split_query_bf16(const float *q, size_t d, uint16_t *hi_out, uint16_t *lo_out) {
    if (!q || !hi_out || !lo_out || d == 0) {
        leann_set_error("leann_split_query_bf16: null %s", !q ? "q" : !hi_out ? "hi_out" : !lo_out ? "lo_out" : "query (d = 0)");
        return LEANN_ERR_INVALID;
    }
    for (size_t j = 0; j < d; j++) {
        hi_out[j] = f32_to_bf16_rne(q[j]);
        lo_out[j] = split_lo(q[j], hi_out[j]);
    }
    return LEANN_OK;
}
