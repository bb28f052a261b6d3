// recompute.hip — the LEANN "no stored vectors" search: embeddings are recomputed on the fly from a
// device-resident encoder and never kept.
//
// Reference path (src/index/recompute.rs:52-123): for every passage, embedding_provider.embed(..)
// (:86-93) -> dot with the query (:96-103) -> stable sort descending (:106) -> take(k) (:109-120).
// The provider's last stage is a dense layer + L2 normalisation (candle.rs:165, :218-225:
// x / max(sqrt(sum x^2), 1e-12)); the transformer in front of it is out of scope (no weights offline),
// so the device-resident "embedding provider" here is:
//     per-passage compact feature  f_i  [h]      bf16   (h = 256: 512 B instead of 3 072 B per passage)
//     encoder weights              W    [h x d]  bf16
//     embedding_i = l2_normalize(W^T f_i)  with f32 accumulation
//
// Search (leann_recompute_search_batch[_device]), per tile of <= 64 queries: G = W Q^T once (project_queries_kernel), then
//   * common shape (h = 256, dims % 128 == 0, one token row per passage): fused_fstat_kernel (recompute_fstat.cuh) — encode GEMM,
//     row norms, feature-space scoring and candidate emission in one persistent kernel; first 16k rows through a score slab +
//     segment top-k (scan.hip) to establish the running k-th best, the rest emits survivors only (fold_candidates_kernel);
//   * other shapes: encode_kernel<CT, FUSED, POOL> below (128 passages x all columns per workgroup, both operands through LDS,
//     masked mean pooling over L token rows in the epilogue) + score slab + segment top-k per chunk.
// Embeddings are never materialised by a search; leann_recompute_encode_device writes them for validation, and
// leann_recompute_build_index builds a graph on a transient copy and keeps only features + norms (recompute-on graph).
#include "common.cuh"
#include "../../include/leann_backend.h"
#include "internal.h"
#include <thread>
#include <cstring>
#include <string>
#include "recompute_fstat.cuh" // fused_fstat_kernel, tile_features_kernel; bf16x8 / f32x16
#include <algorithm>
#include <mutex>
#include <utility>
#include <vector>
#include "bf16.h" // f32_to_bf16_rne

// A launch of a kernel whose dynamic LDS may pass 64 KiB: raise the kernel's limit to the CU's 160 KiB (where the site says so),
// launch, check.  The arguments are converted to the kernel's parameter types.
template <typename... P, typename... A>
static int launch_lds(void (*kernel)(P...), bool raise_limit, unsigned grid, unsigned block, size_t lds, hipStream_t st, A... args) {
    if (raise_limit) HIP_CHECK_RET(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds, st, static_cast<P>(args)...);
    HIP_CHECK_RET(hipGetLastError());
    return LEANN_OK;
}

// ---- synthetic features / weights: the recompute twin of gen.hip -----------------------------------
// f_i[k] = bf16(centre_c[k] + sigma * noise_i[k]),  W[k][j] = bf16(gauss(k, j))  (same hash streams as
// gen.hip with r = h), so normalise(W^T f_i) is the clustered synthetic corpus at bf16 input precision.
#define TAG_P 0x50524F4A00000000ull
#define TAG_C 0x43454E5400000000ull
#define TAG_A 0x4153534700000000ull
#define TAG_N 0x4E4F495300000000ull
#define TAG_F 0x4645415400000000ull /* feature lift */
// r_int == 0: f = bf16(z), z in R^h.   r_int > 0: z in R^r_int (clusters + noise, as gen.hip), f[k] = bf16(sum_m A[k][m] z[m])
// (fmaf chain in increasing m) — features of width h with intrinsic dimension r_int, like real encoder inputs.
__global__ void __launch_bounds__(256) synth_features_kernel(uint64_t seed, uint32_t h, uint32_t r_int, uint32_t n_clusters, float sigma,
                                                             uint32_t stream_id, uint64_t i0, uint64_t n, uint16_t *__restrict__ out) {
    extern __shared__ float s_feat[]; // [h * r_int] lift matrix A, then [r_int] z
    const uint64_t nseed = seed ^ TAG_N ^ ((uint64_t)stream_id * 0x9E3779B97F4A7C15ull);
    if (r_int == 0) {
        for (uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n * h; idx += (uint64_t)gridDim.x * blockDim.x) {
            const uint64_t i = i0 + idx / h;
            const uint32_t k = (uint32_t)(idx % h);
            const uint64_t c = hash3(seed ^ TAG_A, stream_id, i) % n_clusters;
            out[idx] = f32_to_bf16_rne(fmaf(sigma, gauss_ih4(nseed, i, k), gauss_ih4(seed ^ TAG_C, c, k)));
        }
        return;
    }
    float *A = s_feat, *z = s_feat + (size_t)h * r_int;
    for (uint32_t idx = threadIdx.x; idx < h * r_int; idx += blockDim.x) A[idx] = gauss_ih4(seed ^ TAG_F, idx / r_int, idx % r_int);
    for (uint64_t ii = blockIdx.x; ii < n; ii += gridDim.x) {
        const uint64_t i = i0 + ii;
        const uint64_t c = hash3(seed ^ TAG_A, stream_id, i) % n_clusters;
        __syncthreads();
        for (uint32_t m = threadIdx.x; m < r_int; m += blockDim.x)
            z[m] = fmaf(sigma, gauss_ih4(nseed, i, m), gauss_ih4(seed ^ TAG_C, c, m));
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < h; k += blockDim.x) {
            float acc = 0.f;
            for (uint32_t m = 0; m < r_int; m++) acc = fmaf(A[k * r_int + m], z[m], acc);
            out[ii * h + k] = f32_to_bf16_rne(acc);
        }
    }
}
__global__ void synth_weights_kernel(uint64_t seed, uint32_t h, uint32_t d, uint16_t *__restrict__ W /* [h x d] */) {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= h * d) return;
    W[idx] = f32_to_bf16_rne(gauss_ih4(seed ^ TAG_P, idx / d, idx % d));
}
extern "C" int leann_synth_features_device(uint64_t seed, uint32_t h, uint32_t r_int, uint32_t n_clusters, float sigma,
                                           uint32_t stream_id, uint64_t i0, uint64_t n, uint16_t *d_out, void *stream) {
    if (!d_out || h == 0 || n_clusters == 0 || (size_t)(h + 1) * r_int * 4 > 150 * 1024) {
        leann_set_error("leann_synth_features_device: invalid arguments (h=%u r_int=%u)", h, r_int);
        return LEANN_ERR_INVALID;
    }
    if (n == 0) return LEANN_OK;
    const size_t lds = r_int ? ((size_t)h * r_int + r_int) * 4 : 0;
    const uint64_t blocks = r_int ? std::min<uint64_t>(n, 4096) : std::min<uint64_t>((n * h + 255) / 256, 65536);
    return launch_lds(synth_features_kernel, lds > 64 * 1024, (unsigned)blocks, 256, lds, (hipStream_t)stream, seed, h, r_int, n_clusters,
                      sigma, stream_id, i0, n, d_out);
}
extern "C" int leann_synth_weights_device(uint64_t seed, uint32_t h, uint32_t dims, uint16_t *d_out, void *stream) {
    if (!d_out || h == 0 || dims == 0) { leann_set_error("leann_synth_weights_device: invalid arguments"); return LEANN_ERR_INVALID; }
    hipLaunchKernelGGL(synth_weights_kernel, dim3((h * dims + 255) / 256), dim3(256), 0, (hipStream_t)stream, seed, h, dims, d_out);
    HIP_CHECK_RET(hipGetLastError());
    return LEANN_OK;
}

// ---- weights re-tiled for the MFMA B operand: Wp[kstep][col][16] bf16, col padded to CT*32 ------------
__global__ void tile_weights_kernel(const uint16_t *__restrict__ W, uint32_t h, uint32_t d, uint32_t hp, uint32_t dp,
                                    uint16_t *__restrict__ Wp) {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= hp * dp) return;
    const uint32_t ks = idx / (dp * 16), rem = idx % (dp * 16), col = rem / 16, kk = rem % 16, k = ks * 16 + kk;
    Wp[idx] = (k < h && col < d) ? W[(size_t)k * d + col] : (uint16_t)0;
}

// ------------------------------------------------------------------------------------------------
// Query-side projection for the fused search: G = W Q^T  [h x 64] in f32 (k-ordered fmaf chain), split
// into three bf16 pieces g = hi + lo + lo2 (24 mantissa bits: since the features are exactly bf16, the
// three bf16 MFMAs F*hi + F*lo + F*lo2 reproduce the f32 products F*g), tiled like the weights:
// Gp[kstep][piece*64 + q][16].  By associativity  <l2norm(W^T f), q> = <f, W q> / ||W^T f||, so the
// d-dimensional scoring GEMM against materialised embeddings becomes an h-dimensional one fused into
// the encode loop, and the embeddings never leave the registers.
// ------------------------------------------------------------------------------------------------
// Workgroup = 4 rows of W x 64 queries; the queries go through LDS in chunks of 64 columns (coalesced 256-B row pieces, stored
// transposed so that consecutive queries sit in consecutive banks), the W values are wave-uniform.  Each g is still ONE fmaf chain,
// j ascending — the arithmetic did not change, only the access pattern (one thread per (k, q) reading its query row straight from
// global memory touched 64 cache lines per load instruction: 112 us per 64 queries, 0.45 ms per 256).
__global__ void __launch_bounds__(256) project_queries_kernel(const uint16_t *__restrict__ W, uint32_t h, uint32_t hp, uint32_t d,
                                                              const float *__restrict__ Q, uint32_t ldq, uint32_t nq,
                                                              uint16_t *__restrict__ Gp, int by_query_tile, uint32_t q_slots) {
    // q_slots: query slots of the image (64 for encode_kernel; a multiple of 32 up to FSTAT_MAX_QUERIES for fused_fstat_kernel)
    __shared__ float sQ[64][65];
    __shared__ float sW[4][64];
    const uint32_t tid = threadIdx.x, kl = tid >> 6, ql = tid & 63;
    const uint32_t k = blockIdx.x * 4 + kl, q = blockIdx.y * 64 + ql;
    float g = 0.f;
    for (uint32_t j0 = 0; j0 < d; j0 += 64) {
        __syncthreads();
#pragma unroll
        for (int p = 0; p < 4; p++) { // 16 query rows per pass, 4 consecutive columns per thread
            const uint32_t qr = (tid >> 4) + 16 * p, jj = (tid & 15) * 4, qg = blockIdx.y * 64 + qr;
#pragma unroll
            for (int e = 0; e < 4; e++) sQ[jj + e][qr] = (qg < nq && j0 + jj + e < d) ? Q[(size_t)qg * ldq + j0 + jj + e] : 0.f;
        }
        {
            const uint32_t kr = blockIdx.x * 4 + (tid >> 6), jc = j0 + (tid & 63);
            sW[tid >> 6][tid & 63] = (kr < h && jc < d) ? __uint_as_float((uint32_t)W[(size_t)kr * d + jc] << 16) : 0.f;
        }
        __syncthreads();
        const uint32_t lim = min(64u, d - j0);
        if (lim == 64) {
#pragma unroll 16
            for (uint32_t j = 0; j < 64; j++) g = fmaf(sW[kl][j], sQ[j][ql], g);
        } else {
            for (uint32_t j = 0; j < lim; j++) g = fmaf(sW[kl][j], sQ[j][ql], g);
        }
    }
    if (k >= hp || q >= q_slots) return;
    if (!(k < h && q < nq)) g = 0.f;
    const uint16_t hi = f32_to_bf16_rne(g);
    const float r1 = g - __uint_as_float((uint32_t)hi << 16);
    const uint16_t lo = f32_to_bf16_rne(r1);
    const float r2 = r1 - __uint_as_float((uint32_t)lo << 16);
    const uint16_t lo2 = f32_to_bf16_rne(r2);
    const uint32_t ks = k / 16, kk = k % 16;
    uint16_t *base = Gp + (size_t)ks * (q_slots * 3) * 16;
    if (by_query_tile) { // fused_fstat_kernel: Gp[kstep][query tile][piece][32 q][16] — the three pieces of a query tile are contiguous
        base += ((q >> 5) * 96 + (q & 31)) * 16 + kk;
        base[0] = hi;
        base[32 * 16] = lo;
        base[64 * 16] = lo2;
        return;
    }
    base[(0 * 64 + q) * 16 + kk] = hi;
    base[(1 * 64 + q) * 16 + kk] = lo;
    base[(2 * 64 + q) * 16 + kk] = lo2;
}

// ------------------------------------------------------------------------------------------------
// encode_kernel<CT, FUSED, POOL>: 512 threads = 8 waves; workgroup tile = 128 passages x (CT*4*32) columns
// (CT col tiles of 32 per wave, 4 column groups, 2 row halves of 64 passages).  d <= CT*128.
// LDS: sF[128][hp + 8] bf16 (whole K, loaded once) + a 3-slot ring of sW[DP (+192)][16] bf16 k-step slabs + sN / sM / sC.
//   FUSED = false: E = l2norm(F W) stored as f32 (validation / leann_recompute_encode_device)
//   FUSED = true : nothing but S[q][passage] = <f, W q> / ||W^T f|| leaves the workgroup
//   POOL         : masked mean pooling over the L token rows of a passage between the GEMM and the norm
// Its phases are the fragments encode_*.cuh, which encode_blocked_kernel (recompute_blocked.cuh) runs per column block: each is
// stated once and included at its place, so that both kernels keep the device code they had (profiles/encode_fragments.md).
// The kernel's own: the LDS layout, the one block's names (dp, col0, SN_ADD, SCORE) and the normalised store of E.
// ------------------------------------------------------------------------------------------------
template <int CT, bool FUSED, bool POOL>
__global__ void __launch_bounds__(512) encode_kernel(const uint16_t *__restrict__ F, uint64_t n, uint32_t h, uint32_t hp,
                                                     const uint16_t *__restrict__ Wp, uint32_t d, uint32_t ld_out,
                                                     float *__restrict__ E, const uint16_t *__restrict__ Gp, uint32_t nq,
                                                     float *__restrict__ S, uint32_t n_rows_s, uint32_t L,
                                                     const uint8_t *__restrict__ mask, float *__restrict__ norms_out) {
    constexpr bool SCORE = FUSED;               // the fragments' name: the one block is also the block that scores
    constexpr int DP = CT * 128;                // padded columns of W
    constexpr int DPX = DP + (SCORE ? 192 : 0); // + three 64-query pieces of G
    constexpr int RING = 3;                     // k-step slabs in LDS: one being consumed, two in flight
    constexpr int NI = DPX * 2 / 64;            // 1-KiB DMA instructions per k-step slab
    constexpr int PER = (NI + 7) / 8;           // ... per wave (the same count in every wave: counted vmcnt waits)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t fstride = hp + 8; // bf16 elements per sF row
    uint16_t *sF = reinterpret_cast<uint16_t *>(smem);
    uint16_t *sW = sF + 128 * fstride;                              // [RING][DPX][16] linear, swizzled 16-B slots
    float *sN = reinterpret_cast<float *>(sW + RING * DPX * 16);    // [4 col groups][128 rows] partial sum of squares
    float *sM = sN + 4 * 128;                                       // [128] attention mask of the tile's token rows (0/1)
    float *sC = sM + 128;                                           // [128] max(token count, 1e-9) at each passage's first row
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int rhalf = wave >> 2, cgrp = wave & 3;
    const uint64_t row_base = (uint64_t)blockIdx.x * 128;

#include "encode_features.cuh" // the feature tile -> sF
    constexpr uint32_t dp = DP, col0 = 0; // the one block: every column of a k-step slab, from column 0
#include "encode_ring.cuh" // stage_w, frag, acc = 0, accs = 0
    const int st = cgrp >> 1, qt = cgrp & 1;
    const uint32_t nks = hp / 16;
#include "encode_mask.cuh" // sM, sC; its barrier publishes the feature tile
#include "encode_kloop.cuh" // acc = F W, SCORE: accs = G F^T
    __syncthreads(); // every wave is done with the ring (all DMA waited for: a plain barrier)
    constexpr bool SN_ADD = false; // the one block: its sums of squares are the row's
#include "encode_pool.cuh" // POOL: acc = masked mean over the L token rows; sN = the sums of squares
    __syncthreads(); // the sums of squares of every column group are in sN
    if (FUSED) {
#include "encode_score.cuh" // S = accs / nrm
        return;
    }
#pragma unroll
    for (int rt = 0; rt < 2; rt++) {
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {
            const int r = rhalf * 64 + rt * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
            const uint64_t row = row_base + r;
#include "encode_norm.cuh" // nrm
            if (row < n && (r % L) == 0) {
                if (norms_out && cgrp == 0 && l31 == 0) norms_out[row / L] = nrm; // ||W^T f|| before normalisation
#pragma unroll
                for (int ct = 0; ct < CT; ct++) {
                    const uint32_t col = (cgrp * CT + ct) * 32 + l31;
                    if (col < ld_out) E[(size_t)(row / L) * ld_out + col] = col < d ? acc[rt][ct][reg] / nrm : 0.f;
                }
            }
        }
    }
}

#include "recompute_blocked.cuh" // encode_blocked_kernel: the same k-loop over column blocks, for dims > 768

// ------------------------------------------------------------------------------------------------
struct leann_recompute {
    int device = 0;
    const uint16_t *F = nullptr; // borrowed [n x h]
    DeviceBuf<uint16_t> Wp;      // owned, tiled
    DeviceBuf<uint16_t> Wraw;    // owned copy [h x d] (query projection)
    size_t n = 0, h = 0, hp = 0, d = 0, dp = 0, ld = 0;
    uint64_t key_offset = 0;
    int ct = 0;                     // dims <= 768: column tiles of the one block (encode_kernel<ct, ..>)
    EncodeBlocks blocks = {};       // dims > 768: the column blocks of encode_blocked_kernel (encode_plan.h)
    int ctb_max = 0;                // ... and the widest of them, which sizes the LDS ring
    uint32_t L = 1;                 // token rows per passage (masked mean pooling), 1 | 2 | 4 | 8
    const uint8_t *mask = nullptr;  // borrowed [n x L] attention mask or null (all ones)
    float last_ms[3] = {0, 0, 0}; // encode, score, top-k of the last search call (HIP events)
    // search scratch, grown on demand and kept (hipMalloc / hipFree of ~1 GB per call costs 2-30 ms depending on the box);
    // one search at a time per handle
    std::mutex mu;
    DeviceBuf<float> sS;
    DeviceBuf<uint16_t> sGp;
    DeviceBuf<uint64_t> sCandA, sCandB, sBest;
    DeviceBuf<uint4> Ft;            // fragment-major copy of F (tile_features_kernel), made by the first exhaustive search
    DeviceBuf<uint16_t> ownF;       // leann_recompute_create_host: the handle's own copy of the features
    DeviceBuf<unsigned char> sEmit; // the emission block of topk_plan.h, FSTAT_MAX_QUERIES slots
    // sharded form (leann_recompute_create_sharded): the passages live in `parts` (consecutive position ranges, possibly on different
    // devices); this handle owns only the gather block and the per-part staging
    struct Part {
        const leann_recompute *r = nullptr;
        hipStream_t st = nullptr;
        hipEvent_t done = nullptr;
        DeviceBuf<unsigned char> stage; // remote parts: [queries | keys | scores | counts | mask slice] on the part's device
    };
    std::vector<Part> parts;
    DeviceBuf<unsigned char> gather; // [n_parts x {keys | scores | counts}] on `device`
    hipEvent_t ev_q = nullptr;
};

// the feature-stationary fused kernel serves the common shape (one token row per passage, h = 256, dims a multiple of 128);
// LEANN_DEBUG_FUSED_V1 forces the general kernel (tests compare the two)
static bool use_fstat(const leann_recompute *r) {
    return r->L == 1 && !r->mask && r->h == 256 && r->dp % 128 == 0 && !leann_knobs().fused_v1;
}

// The general encode kernels this file compiles, one row per kernel, the key and the instantiation written from the same template
// arguments.  ct = 0: encode_blocked_kernel, which takes its block widths at run time.
template <typename K>
struct EncodeRow {
    int ct;
    bool fused, pool;
    K kernel;
};
using EncodeKernel = decltype(&encode_kernel<1, false, false>);
using EncodeBlockedKernel = decltype(&encode_blocked_kernel<false, false>);
template <int CT, bool FUSED, bool POOL>
static constexpr EncodeRow<EncodeKernel> encode_row() { return {CT, FUSED, POOL, encode_kernel<CT, FUSED, POOL>}; }
template <bool FUSED, bool POOL>
static constexpr EncodeRow<EncodeBlockedKernel> encode_blocked_row() { return {0, FUSED, POOL, encode_blocked_kernel<FUSED, POOL>}; }
#define ENCODE_FORMS(CT) encode_row<CT, false, false>(), encode_row<CT, false, true>(), encode_row<CT, true, false>(), encode_row<CT, true, true>()
static constexpr EncodeRow<EncodeKernel> encode_rows[] = {ENCODE_FORMS(1), ENCODE_FORMS(2), ENCODE_FORMS(3), ENCODE_FORMS(4), ENCODE_FORMS(6)};
#undef ENCODE_FORMS
static constexpr EncodeRow<EncodeBlockedKernel> encode_blocked_rows[] = {encode_blocked_row<false, false>(), encode_blocked_row<false, true>(),
                                                                         encode_blocked_row<true, false>(), encode_blocked_row<true, true>()};
template <typename K, size_t N>
static constexpr K encode_find(const EncodeRow<K> (&rows)[N], int ct, bool fused, bool pool) {
    for (const EncodeRow<K> &row : rows)
        if (row.ct == ct && row.fused == fused && row.pool == pool) return row.kernel;
    return nullptr;
}
static constexpr bool encode_rows_match_plan() { // the widths encode_plan may choose, in all four forms, and no others
    for (int ct = 0; ct < 16; ct++)
        for (int form = 0; form < 4; form++)
            if ((encode_find(encode_rows, ct, (form & 2) != 0, (form & 1) != 0) != nullptr) != encode_ct_compiled(ct)) return false;
    return true;
}
static_assert(encode_rows_match_plan(), "encode_rows and encode_ct_compiled (encode_plan.h) list different widths");

static int launch_encode(const leann_recompute *r, uint64_t row0, uint64_t rows, float *E, hipStream_t st,
                         const uint16_t *Gp = nullptr, uint32_t nq = 0, float *S = nullptr, float *norms = nullptr,
                         const CandEmit *emit = nullptr, const uint32_t *idx = nullptr) {
    const bool fused = Gp != nullptr;
    if (idx && !(fused && use_fstat(r))) {
        leann_set_error("recompute: a row list needs the fused feature-stationary kernel");
        return LEANN_ERR_INVALID;
    }
    if (fused && use_fstat(r)) {
        // features stationary in registers (the common shape: h = 256, dims = 384 / 768)
        const size_t lds2 = 2 * 16 * 128 * 32 + 4 * 64 * 4 + FSTAT_MAX_QUERIES * 4; // two 64-KiB sub-slice buffers + per-wave norm exchange + thresholds
        const uint64_t unit_rows = 4 * LEANN_FSTAT_RB * 32, units = (rows + unit_rows - 1) / unit_rows; // NWV * RB * 32 passages per unit
        int cus = 256;
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, r->device);
        const unsigned grid2 = (unsigned)std::min<uint64_t>(units, (uint64_t)cus);
        const CandEmit em = emit ? *emit : CandEmit{};
        if (idx) // rows [row0, row0 + rows) of the LIST: passage i = row idx[i] of the row-major features
            return launch_lds(fused_fstat_kernel<16, false, true>, true, grid2, 256, lds2, st, r->F, rows, r->Wp.p, r->dp, Gp, nq, S, rows, em,
                              idx + row0);
        if (r->Ft)
            return launch_lds(fused_fstat_kernel<16, true>, true, grid2, 256, lds2, st, reinterpret_cast<const uint16_t *>(r->Ft.p) + row0 * r->h,
                              rows, r->Wp.p, r->dp, Gp, nq, S, rows, em, nullptr);
        return launch_lds(fused_fstat_kernel<16, false>, true, grid2, 256, lds2, st, r->F + row0 * r->h, rows, r->Wp.p, r->dp, Gp, nq, S, rows, em,
                          nullptr);
    }
    // row0 / rows count PASSAGES; the kernel works on token rows (L per passage, tiles of 128 token rows)
    const uint64_t tok0 = row0 * r->L, toks = rows * r->L;
    const unsigned grid = (unsigned)((toks + 127) / 128);
    const uint16_t *F = r->F + tok0 * r->h;
    const uint8_t *mk = r->mask ? r->mask + tok0 : nullptr;
    const bool pool = r->L > 1 || r->mask != nullptr;
    if (r->blocks.n) // dims > 768: column blocks, the LDS ring sized by the widest one
        return launch_lds(encode_find(encode_blocked_rows, 0, fused, pool), true, grid, 512,
                          encode_lds_bytes(r->hp, (size_t)r->ctb_max * 128, fused), st, F, toks, r->h, r->hp, r->Wp.p, r->d, r->dp, r->ld, E, Gp,
                          nq, S, rows, r->L, mk, norms, r->blocks);
    const EncodeKernel kernel = encode_find(encode_rows, r->ct, fused, pool);
    if (!kernel) {
        leann_set_error("recompute: unsupported dims %zu", r->d);
        return LEANN_ERR_INVALID;
    }
    return launch_lds(kernel, true, grid, 512, encode_lds_bytes(r->hp, r->dp, fused), st, F, toks, r->h, r->hp, r->Wp.p, r->d, r->ld, E, Gp, nq, S,
                      rows, r->L, mk, norms);
}

extern "C" int leann_recompute_create(const uint16_t *d_features, size_t n, size_t h, const uint16_t *d_weights, size_t dims,
                                      int device, uint64_t key_offset, leann_recompute **out) {
    if (!out || (n && !d_features) || !d_weights || h == 0 || dims == 0 || dims > LEANN_ENCODE_MAX_DIMS || n >= (1ull << 32)) {
        leann_set_error("leann_recompute_create: invalid arguments (n=%zu h=%zu dims=%zu; dims <= %d)", n, h, dims, LEANN_ENCODE_MAX_DIMS);
        return LEANN_ERR_INVALID;
    }
    if (int rc = leann_internal_check_device(device)) return rc;
    HIP_CHECK_RET(hipSetDevice(device));
    // columns -> blocks of compiled widths (encode_plan.h); the LDS check is on the widest BLOCK, not on dp
    const EncodePlan plan = encode_plan(h, dims);
    if (!plan.ok) {
        leann_set_error("recompute: feature width %zu x dims %zu exceeds the 160 KiB LDS tile", h, dims);
        return LEANN_ERR_INVALID;
    }
    std::unique_ptr<leann_recompute, void (*)(leann_recompute *)> r(new leann_recompute(), leann_recompute_close); // an error return closes it
    r->device = device;
    r->F = d_features;
    r->n = n;
    r->h = h;
    r->hp = (h + 15) / 16 * 16;
    r->d = dims;
    r->ld = (dims + 3) & ~(size_t)3;
    r->dp = plan.dp;
    r->ctb_max = plan.ctb_max;
    if (plan.nblk == 1) r->ct = plan.ctb[0];
    else {
        r->blocks.n = (uint32_t)plan.nblk;
        for (int b = 0; b < plan.nblk; b++) r->blocks.set((uint32_t)b, (uint32_t)plan.ctb[b]);
    }
    r->key_offset = key_offset;
    if (r->Wp.alloc(r->hp * r->dp) || r->Wraw.alloc(h * dims)) return LEANN_ERR_DEVICE;
    HIP_CHECK_RET(hipMemcpy(r->Wraw, d_weights, h * dims * 2, hipMemcpyDeviceToDevice));
    const uint32_t total = (uint32_t)(r->hp * r->dp);
    hipLaunchKernelGGL(tile_weights_kernel, dim3((total + 255) / 256), dim3(256), 0, nullptr, d_weights, (uint32_t)h, (uint32_t)dims,
                       (uint32_t)r->hp, (uint32_t)r->dp, r->Wp.p);
    HIP_CHECK_RET(hipGetLastError());
    HIP_CHECK_RET(hipDeviceSynchronize());
    *out = r.release();
    return LEANN_OK;
}
// Token-level provider: features [n x L x h], attention mask [n x L] (0 = padding) -> masked mean pooling
// (candle.rs:191-216) between the dense layer and the normalisation.
extern "C" int leann_recompute_create_pooled(const uint16_t *d_features, const uint8_t *d_mask, size_t n, size_t tokens_per_passage,
                                             size_t h, const uint16_t *d_weights, size_t dims, int device, uint64_t key_offset,
                                             leann_recompute **out) {
    if (tokens_per_passage != 1 && tokens_per_passage != 2 && tokens_per_passage != 4 && tokens_per_passage != 8) {
        leann_set_error("leann_recompute_create_pooled: tokens_per_passage must be 1, 2, 4 or 8 (got %zu)", tokens_per_passage);
        return LEANN_ERR_INVALID;
    }
    int rc = leann_recompute_create(d_features, n, h, d_weights, dims, device, key_offset, out);
    if (rc) return rc;
    (*out)->L = (uint32_t)tokens_per_passage;
    (*out)->mask = d_mask;
    return LEANN_OK;
}
// Host-memory twins of create / search (SURVEY.md §8b "Recompute boundary": plain host pointers in, results out).
extern "C" int leann_recompute_create_host(const uint16_t *features, size_t n, size_t h, const uint16_t *weights, size_t dims,
                                           int device, uint64_t key_offset, leann_recompute **out) {
    if (!out || (n && !features) || !weights || h == 0 || dims == 0) {
        leann_set_error("leann_recompute_create_host: null/zero argument");
        return LEANN_ERR_INVALID;
    }
    if (dims > LEANN_ENCODE_MAX_DIMS) { // before any device work, as leann_recompute_create
        leann_set_error("leann_recompute_create_host: invalid arguments (dims=%zu; dims <= %d)", dims, LEANN_ENCODE_MAX_DIMS);
        return LEANN_ERR_INVALID;
    }
    if (int rc = leann_internal_check_device(device)) return rc;
    HIP_CHECK_RET(hipSetDevice(device));
    DeviceBuf<uint16_t> dF, dW; // dW: copied and re-tiled by create, this call's own to the end
    if (dF.alloc(std::max<size_t>(n * h, 8)) || dW.alloc(h * dims)) return LEANN_ERR_DEVICE;
    int rc = LEANN_OK;
    if ((n && hipMemcpy(dF, features, n * h * 2, hipMemcpyHostToDevice) != hipSuccess) ||
        hipMemcpy(dW, weights, h * dims * 2, hipMemcpyHostToDevice) != hipSuccess) {
        leann_set_error("H2D copy of the encoder inputs failed");
        rc = LEANN_ERR_DEVICE;
    }
    if (rc == LEANN_OK) rc = leann_recompute_create(dF, n, h, dW, dims, device, key_offset, out);
    if (rc != LEANN_OK) return rc;
    (*out)->ownF = std::move(dF);
    return LEANN_OK;
}
extern "C" int leann_recompute_search_batch(const leann_recompute *r, const float *queries, size_t nq, size_t top_k,
                                            const uint8_t *allow_mask, uint64_t *keys, float *scores, uint32_t *counts) {
    if (!r || !queries || !keys || !scores || !counts || top_k == 0) {
        leann_set_error("leann_recompute_search_batch: null/zero argument");
        return LEANN_ERR_INVALID;
    }
    if (nq == 0) return LEANN_OK;
    HIP_CHECK_RET(hipSetDevice(r->device));
    const size_t nmask = allow_mask ? (r->n + 7) / 8 : 0;
    DeviceBuf<unsigned char> buf; // [queries | keys | scores | counts | mask]
    const size_t oq = 0, ok = oq + nq * r->d * 4, os = ok + nq * top_k * 8, oc = os + nq * top_k * 4, om = (oc + nq * 4 + 15) & ~(size_t)15;
    int rc = buf.alloc(om + nmask + 16);
    if (rc) return rc;
    if (hipMemcpy(buf + oq, queries, nq * r->d * 4, hipMemcpyHostToDevice) != hipSuccess ||
        (nmask && hipMemcpy(buf + om, allow_mask, nmask, hipMemcpyHostToDevice) != hipSuccess)) {
        leann_set_error("H2D copy of the queries failed");
        rc = LEANN_ERR_DEVICE;
    }
    if (rc == LEANN_OK)
        rc = leann_recompute_search_batch_device(r, (const float *)(buf + oq), nq, top_k, nmask ? buf + om : nullptr, (uint64_t *)(buf + ok),
                                                 (float *)(buf + os), (uint32_t *)(buf + oc), nullptr);
    if (rc == LEANN_OK && (hipDeviceSynchronize() != hipSuccess || hipMemcpy(keys, buf + ok, nq * top_k * 8, hipMemcpyDeviceToHost) != hipSuccess ||
                           hipMemcpy(scores, buf + os, nq * top_k * 4, hipMemcpyDeviceToHost) != hipSuccess ||
                           hipMemcpy(counts, buf + oc, nq * 4, hipMemcpyDeviceToHost) != hipSuccess)) {
        leann_set_error("recompute search: device error: %s", hipGetErrorString(hipGetLastError()));
        rc = LEANN_ERR_DEVICE;
    }
    return rc;
}

// ---- sharded recompute search -------------------------------------------------------------------
// RecomputeSearcher::search scores EVERY passage (recompute.rs:86-103); the top-k of a union is the top-k of the per-part top-ks, so the
// passages split into consecutive position ranges, every part runs its own fused scan (concurrently: one host thread per part, the
// parts may sit on different devices) and the per-part lists are merged by (score descending, key ascending) — the order of the
// reference's stable sort (recompute.rs:106).  Per-passage arithmetic does not depend on a passage's neighbours in a tile, so the
// answer equals the unsharded handle's bit for bit (tests/test_gpu_shard.py).
extern "C" int leann_recompute_create_sharded(const leann_recompute *const *parts, size_t n_parts, leann_recompute **out) {
    if (!parts || !out || n_parts == 0 || n_parts > 64) { leann_set_error("leann_recompute_create_sharded: invalid arguments"); return LEANN_ERR_INVALID; }
    *out = nullptr;
    for (size_t g = 0; g < n_parts; g++) {
        const leann_recompute *p = parts[g];
        if (!p || !p->parts.empty() || p->d != parts[0]->d || p->h != parts[0]->h || p->L != parts[0]->L ||
            (g && p->key_offset != parts[g - 1]->key_offset + parts[g - 1]->n) || (g && ((p->key_offset - parts[0]->key_offset) & 7))) {
            leann_set_error("leann_recompute_create_sharded: part %zu is null, itself sharded, of another shape, or does not continue part %zu's "
                            "position range at a multiple of 8", g, g ? g - 1 : 0);
            return LEANN_ERR_INVALID;
        }
    }
    leann_recompute *r = new leann_recompute();
    r->device = parts[0]->device;
    r->d = parts[0]->d; r->h = parts[0]->h; r->hp = parts[0]->hp; r->dp = parts[0]->dp; r->ld = parts[0]->ld; r->L = parts[0]->L;
    r->key_offset = parts[0]->key_offset;
    bool ok = hipSetDevice(r->device) == hipSuccess && hipEventCreateWithFlags(&r->ev_q, hipEventDisableTiming) == hipSuccess;
    for (size_t g = 0; ok && g < n_parts; g++) {
        leann_recompute::Part pt;
        pt.r = parts[g];
        r->n += parts[g]->n;
        ok = hipSetDevice(parts[g]->device) == hipSuccess && hipStreamCreateWithFlags(&pt.st, hipStreamNonBlocking) == hipSuccess &&
             hipEventCreateWithFlags(&pt.done, hipEventDisableTiming) == hipSuccess;
        r->parts.push_back(std::move(pt));
    }
    (void)hipSetDevice(r->device);
    if (!ok) {
        leann_set_error("leann_recompute_create_sharded: stream / event creation failed: %s", hipGetErrorString(hipGetLastError()));
        leann_recompute_close(r);
        return LEANN_ERR_DEVICE;
    }
    *out = r;
    return LEANN_OK;
}

static int sharded_recompute_search(leann_recompute *r, const float *d_queries, size_t nq, size_t top_k, const uint8_t *d_allow_mask,
                                    uint64_t *d_keys, float *d_scores, uint32_t *d_counts, hipStream_t st) {
    const size_t G = r->parts.size();
    if (G * top_k > 12288) { leann_set_error("sharded recompute search: parts x top_k = %zu x %zu exceeds the merge kernel's 12288 entries", G, top_k); return LEANN_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(r->mu); // one search at a time per handle, like a plain handle's scratch
    HIP_CHECK_RET(hipSetDevice(r->device));
    const size_t okeys = 0, oscores = nq * top_k * 8, ocounts = nq * top_k * 12, blk = (nq * top_k * 12 + nq * 4 + 15) & ~(size_t)15;
    if (int rc = r->gather.grow(G * blk)) return rc;
    HIP_CHECK_RET(hipEventRecord(r->ev_q, st)); // queries (and the mask) are ready
    std::vector<int> rcs(G, LEANN_OK);
    std::vector<std::string> errs(G);
    auto run_part = [&](size_t g) {
        leann_recompute::Part &pt = r->parts[g];
        const leann_recompute *p = pt.r;
        auto fail = [&](const char *what) { leann_set_error("sharded recompute search, part %zu: %s failed: %s", g, what, hipGetErrorString(hipGetLastError())); return (int)LEANN_ERR_DEVICE; };
        if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice");
        if (hipStreamWaitEvent(pt.st, r->ev_q, 0) != hipSuccess) return fail("hipStreamWaitEvent");
        const bool remote = p->device != r->device || leann_knobs().force_remote;
        const size_t mask_off = (size_t)((p->key_offset - r->key_offset) / 8), mask_b = d_allow_mask ? (p->n + 7) / 8 : 0;
        const float *q = d_queries;
        const uint8_t *mask = d_allow_mask ? d_allow_mask + mask_off : nullptr;
        unsigned char *outb = r->gather + g * blk;
        if (remote) { // queries (and the part's slice of the mask) travel to the part's device, its lists travel back
            const size_t oq = 0, ob = (nq * r->d * 4 + 15) & ~(size_t)15, om = ob + blk, need = om + mask_b + 16;
            if (int rc = pt.stage.grow(need)) return rc;
            if (hipMemcpyPeerAsync(pt.stage + oq, p->device, d_queries, r->device, nq * r->d * 4, pt.st) != hipSuccess) return fail("peer copy of the queries");
            if (mask_b && hipMemcpyPeerAsync(pt.stage + om, p->device, d_allow_mask + mask_off, r->device, mask_b, pt.st) != hipSuccess) return fail("peer copy of the mask");
            q = (const float *)(pt.stage + oq);
            mask = mask_b ? pt.stage + om : nullptr;
            outb = pt.stage + ob;
        }
        int rc = leann_recompute_search_batch_device(p, q, nq, top_k, mask, (uint64_t *)(outb + okeys), (float *)(outb + oscores),
                                                     (uint32_t *)(outb + ocounts), pt.st);
        if (rc) return rc;
        if (remote && hipMemcpyPeerAsync(r->gather + g * blk, r->device, outb, p->device, blk, pt.st) != hipSuccess) return fail("peer copy of the results");
        if (hipEventRecord(pt.done, pt.st) != hipSuccess) return fail("hipEventRecord");
        return (int)LEANN_OK;
    };
    std::vector<std::thread> th;
    for (size_t g = 1; g < G; g++)
        th.emplace_back([&, g] { rcs[g] = run_part(g); if (rcs[g]) errs[g] = leann_last_error(); });
    rcs[0] = run_part(0);
    if (rcs[0]) errs[0] = leann_last_error();
    for (auto &t : th) t.join();
    (void)hipSetDevice(r->device);
    for (size_t g = 0; g < G; g++)
        if (rcs[g]) { leann_set_error("%s", errs[g].c_str()); return rcs[g]; }
    for (size_t g = 0; g < G; g++) HIP_CHECK_RET(hipStreamWaitEvent(st, r->parts[g].done, 0));
    r->last_ms[0] = r->last_ms[1] = r->last_ms[2] = 0.f;
    for (size_t g = 0; g < G; g++)
        for (int i = 0; i < 3; i++) r->last_ms[i] = std::max(r->last_ms[i], r->parts[g].r->last_ms[i]);
    return leann_internal_merge_strided(r->gather + okeys, r->gather + oscores, r->gather + ocounts, blk, blk, blk, G, nq, top_k, top_k, 1, d_keys,
                                        d_scores, d_counts, st);
}

extern "C" void leann_recompute_close(leann_recompute *r) {
    if (!r) return;
    for (auto &pt : r->parts) { // (the parts themselves are borrowed)
        (void)hipSetDevice(pt.r ? pt.r->device : r->device);
        if (pt.st) { (void)hipStreamSynchronize(pt.st); (void)hipStreamDestroy(pt.st); }
        if (pt.done) (void)hipEventDestroy(pt.done);
        pt.stage.reset(); // here: the part's device is current
    }
    if (!r->parts.empty()) (void)hipSetDevice(r->device);
    if (r->ev_q) (void)hipEventDestroy(r->ev_q);
    delete r; // the handle's own buffers go with it
}
extern "C" size_t leann_recompute_len(const leann_recompute *r) { return r ? r->n : 0; }
extern "C" int leann_recompute_last_timing(const leann_recompute *r, float *ms3) {
    if (!r || !ms3) { leann_set_error("leann_recompute_last_timing: null argument"); return LEANN_ERR_INVALID; }
    ms3[0] = r->last_ms[0]; ms3[1] = r->last_ms[1]; ms3[2] = r->last_ms[2];
    return LEANN_OK;
}

// materialise the embeddings of rows [row0, row0 + rows) into d_out [rows x ld] (tests / validation)
extern "C" int leann_recompute_encode_device(const leann_recompute *r, uint64_t row0, uint64_t rows, float *d_out, void *stream) {
    if (!r || !d_out || row0 + rows > r->n) { leann_set_error("leann_recompute_encode_device: invalid arguments"); return LEANN_ERR_INVALID; }
    if (!r->parts.empty()) { leann_set_error("leann_recompute_encode_device: a sharded handle holds no features of its own (encode through its parts)"); return LEANN_ERR_UNSUPPORTED; }
    if (rows == 0) return LEANN_OK;
    HIP_CHECK_RET(hipSetDevice(r->device));
    return launch_encode(r, row0, rows, d_out, (hipStream_t)stream);
}

// RecomputeSearcher::search arithmetic for a batch of queries — recompute.rs:86-109 on the GPU.
// Per tile of <= 64 queries: G = W Q^T once, then per chunk of passages ONE fused kernel (encode GEMM,
// row norms, feature-space scoring) + segment top-k; the embeddings are never written anywhere.
static int recompute_search_impl(const leann_recompute *r, const float *d_queries, size_t nq, size_t top_k, const uint8_t *d_allow_mask,
                                 uint64_t *d_keys, float *d_scores, uint32_t *d_counts, void *stream, const uint32_t *idx = nullptr,
                                 size_t n_list = 0);
extern "C" int leann_recompute_search_batch_device(const leann_recompute *r, const float *d_queries, size_t nq, size_t top_k,
                                                   const uint8_t *d_allow_mask, uint64_t *d_keys, float *d_scores,
                                                   uint32_t *d_counts, void *stream) {
    if (!r || !d_queries || !d_keys || !d_scores || !d_counts || top_k == 0 || top_k > 1024) {
        leann_set_error("leann_recompute_search_batch_device: invalid arguments");
        return LEANN_ERR_INVALID;
    }
    if (nq == 0) return LEANN_OK;
    if (!r->parts.empty())
        return sharded_recompute_search(const_cast<leann_recompute *>(r), d_queries, nq, top_k, d_allow_mask, d_keys, d_scores, d_counts, (hipStream_t)stream);
    HIP_CHECK_RET(hipSetDevice(r->device));
    // The early filter of recompute.rs:62-79: the reference fetches, and therefore embeds, only the passages that pass the filter.
    // A selective mask is compacted into the list of allowed positions and only those rows go through the fused kernel (same
    // per-passage arithmetic, so the same scores as the masked pass over everything); LEANN_RECOMPUTE_NO_LIST=1 keeps the masked pass.
    ScratchLease<uint32_t> list;
    size_t n_list = 0;
    if (d_allow_mask && use_fstat(r) && r->n < (1ull << 32) && !leann_knobs().no_list) {
        int rc = leann_internal_compact_allow(d_allow_mask, r->n, &list, &n_list, (hipStream_t)stream);
        if (rc != LEANN_OK) return rc;
        if (n_list > r->n / 2) { // barely selective: the masked pass reads the fragment-major feature copy and skips the gather
            list.reset(); // (compact_allow synchronised the stream)
        } else if (!list) { // nothing allowed: an empty list still needs a non-null marker for the list path
            if (int e = list.acquire(1)) return e;
        }
    }
    int rc = recompute_search_impl(r, d_queries, nq, top_k, d_allow_mask, d_keys, d_scores, d_counts, stream, list, n_list);
    if (list) (void)hipStreamSynchronize((hipStream_t)stream); // before the lease ends (already idle unless an error cut the search short)
    return rc;
}
static int recompute_search_impl(const leann_recompute *r, const float *d_queries, size_t nq, size_t top_k, const uint8_t *d_allow_mask,
                                 uint64_t *d_keys, float *d_scores, uint32_t *d_counts, void *stream, const uint32_t *idx, size_t n_list) {
    hipStream_t st = (hipStream_t)stream;
    const size_t N = idx ? n_list : r->n; // passages of this search (idx: the allowed ones, keys are list indices until the finalize step)
    if (idx) d_allow_mask = nullptr;
    const uint32_t k = (uint32_t)top_k;
    leann_recompute *rw = const_cast<leann_recompute *>(r);
    std::lock_guard<std::mutex> scratch_lock(rw->mu);
    if (use_fstat(r) && !idx && !rw->Ft && r->n >= 4096 && !leann_knobs().no_tiled) {
        // first exhaustive search on this handle: keep a fragment-major copy of the features (+ n * h * 2 bytes; if HBM is short
        // the kernel reads the caller's row-major array instead, ~10 % slower)
        const uint64_t n_pad = (r->n + 255) / 256 * 256 + 256;
        if (rw->Ft.alloc(n_pad * r->h * 2 / sizeof(uint4)) == LEANN_OK) {
            hipLaunchKernelGGL(tile_features_kernel, dim3(4096), dim3(256), 0, st, r->F, (uint64_t)r->n, (uint32_t)r->h, n_pad, rw->Ft.p);
            HIP_CHECK_RET(hipGetLastError());
        }
    }
    // queries per pass over the passages: the encode GEMM is shared by all of them (fused_fstat_kernel: up to 256, one G sub-slice
    // per 32 queries and unit); the general kernel is built for 64
    const size_t QT = use_fstat(r) ? FSTAT_MAX_QUERIES : 64;
    const TopkShape shape = topk_shape_recompute(N, nq, k, QT);
    if (int e = rw->sGp.grow(r->hp * QT * 3 + 512)) return e; // + the fourth (unused) KiB piece of the last k-step
    uint16_t *Gp = rw->sGp;
    // only the feature-stationary kernel emits; a candidate list that overflows (adversarial score order, e.g. ascending) makes
    // the call repeat on the slab schedule
    for (bool emit = use_fstat(r) && !leann_knobs().no_emit;; emit = false) {
        TopkRun run{topk_plan(shape, emit)};
        const TopkPlan &p = run.plan;
        if (int e = rw->sS.grow(QT * p.slab_rows)) return e;
        if (rw->sCandA.grow(nq * p.cand_len) || rw->sCandB.grow(nq * p.cand_len) || rw->sBest.grow(nq * k)) return LEANN_ERR_DEVICE;
        if (p.emit)
            if (int e = rw->sEmit.grow(p.emit_bytes)) return e;
        const size_t n_chunks = p.chunks.size(), n_tiles = (nq + QT - 1) / QT;
        struct EventSet { // destroyed on every exit, including the HIP_CHECK_RET returns below
            std::vector<hipEvent_t> v;
            ~EventSet() { for (auto &e : v) if (e) (void)hipEventDestroy(e); }
        } evset;
        evset.v.assign(n_tiles * n_chunks * 3 + 1, nullptr);
        std::vector<hipEvent_t> &evs = evset.v;
        for (auto &e : evs) HIP_CHECK_RET(hipEventCreate(&e));
        run.S = rw->sS, run.candA = rw->sCandA, run.candB = rw->sCandB, run.best = rw->sBest, run.emit_block = rw->sEmit;
        run.nq = nq, run.k = k, run.allow = d_allow_mask, run.st = st, run.done = evs.back();
        int rc = leann_internal_topk_begin(run);
        size_t ei = 0;
        for (size_t q0 = 0; q0 < nq && rc == LEANN_OK; q0 += QT) {
            const uint32_t nqt = (uint32_t)std::min<size_t>(QT, nq - q0);
            const uint32_t q_slots = use_fstat(r) ? (nqt + 31) / 32 * 32 : 64; // fused_fstat_kernel sizes its G image by 32-query tiles
            hipLaunchKernelGGL(project_queries_kernel, dim3((unsigned)((r->hp + 3) / 4), (unsigned)((q_slots + 63) / 64)), dim3(256), 0, st, r->Wraw, (uint32_t)r->h,
                               (uint32_t)r->hp, (uint32_t)r->d, d_queries + q0 * r->d, (uint32_t)r->d, nqt, Gp, use_fstat(r) ? 1 : 0, q_slots);
            for (size_t c = 0; c < n_chunks && rc == LEANN_OK; c++) {
                (void)hipEventRecord(evs[ei++], st);
                const CandEmit em = run.chunk_emit(c);
                rc = launch_encode(r, p.chunks[c].first, p.chunks[c].second, nullptr, st, Gp, nqt, run.S, nullptr, &em, idx);
                (void)hipEventRecord(evs[ei++], st);
                if (rc == LEANN_OK) rc = leann_internal_topk_select_chunk(run, c, q0, nqt);
                (void)hipEventRecord(evs[ei++], st);
            }
        }
        bool overflowed = false;
        if (rc == LEANN_OK) rc = leann_internal_topk_finish(run, r->key_offset, idx, 0, d_keys, d_scores, d_counts, &overflowed);
        else (void)hipStreamSynchronize(st);
        rw->last_ms[0] = rw->last_ms[1] = rw->last_ms[2] = 0.f;
        float ms = 0.f;
        for (size_t i = 0; i + 2 < ei + 1 && rc == LEANN_OK; i += 3) {
            if (hipEventElapsedTime(&ms, evs[i], evs[i + 1]) == hipSuccess) rw->last_ms[0] += ms;     // fused encode + score
            if (hipEventElapsedTime(&ms, evs[i + 1], evs[i + 2]) == hipSuccess) rw->last_ms[2] += ms; // segment top-k
        }
        if (ei >= 3 && rc == LEANN_OK && hipEventElapsedTime(&ms, evs[ei - 1], evs[ei]) == hipSuccess) rw->last_ms[2] += ms;
        if (rc != LEANN_OK || !overflowed) return rc;
    }
}

// ================================================================================================
// Recompute-on GRAPH search (the LEANN idea proper: a graph index whose distances are recomputed from the
// encoder inputs instead of stored vectors).  The graph is built once on transiently materialised embeddings;
// afterwards the index keeps only the graph, the bf16 features and one f32 per passage (||W^T f||):
//     dist(q, i) = 1 - <f_i, W q> / ||W^T f_i||   ==   1 - <l2norm(W^T f_i), q>
// 520 B per evaluated neighbour instead of 3 072 B (h = 256, d = 768).  The traversal kernel is the same
// (search.cuh, FEAT instantiation); queries are projected once per batch (g = W q, f32 MFMA).
// ================================================================================================
__global__ void pack_feature_rows_kernel(const uint16_t *__restrict__ F, const float *__restrict__ norms, uint64_t n, uint32_t h,
                                         uint32_t hp4, uint32_t row_bytes, unsigned char *__restrict__ out) {
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; // (row, element) incl. the norm slot
    const uint32_t per = hp4 + 2;                                         // hp4 bf16 + one f32 (= 2 bf16 slots)
    if (idx >= n * per) return;
    const uint64_t row = idx / per;
    const uint32_t e = (uint32_t)(idx % per);
    unsigned char *dst = out + row * row_bytes;
    if (e < hp4) reinterpret_cast<uint16_t *>(dst)[e] = e < h ? F[row * h + e] : (uint16_t)0;
    else if (e == hp4 && row_bytes >= 2 * hp4 + 4) *reinterpret_cast<float *>(dst + 2 * (size_t)hp4) = norms[row]; // (split layout: no slot)
}
// the inline file / export form [features | f32 norm | pad] of an index whose device rows are split (GraphView::norms)
size_t leann_internal_feat_file_row_bytes(const GraphView &g) { return g.norms ? ((2 * (size_t)g.feat_h + 4 + 7) & ~(size_t)7) : g.row_bytes; }
int leann_internal_feat_rows_to_host(const leann_backend *h, size_t r0, size_t rows, unsigned char *out) {
    const size_t fb = leann_internal_feat_file_row_bytes(h->g);
    if (!h->g.norms) {
        HIP_CHECK_RET(hipMemcpy(out, reinterpret_cast<const unsigned char *>(h->g.X) + r0 * h->g.row_bytes, rows * fb, hipMemcpyDeviceToHost));
        return LEANN_OK;
    }
    // contiguous device reads, interleaved on the host (a 2-D copy of 4-byte columns is one tiny DMA per row)
    const size_t fw = 2 * (size_t)h->g.feat_h, slab = (size_t)1 << 20;
    std::vector<unsigned char> fr(std::min(slab, std::max<size_t>(rows, 1)) * fw);
    std::vector<float> nr(std::min(slab, std::max<size_t>(rows, 1)));
    for (size_t s0 = 0; s0 < rows; s0 += slab) {
        const size_t m = std::min(slab, rows - s0);
        HIP_CHECK_RET(hipMemcpy(fr.data(), reinterpret_cast<const unsigned char *>(h->g.X) + (r0 + s0) * h->g.row_bytes, m * fw, hipMemcpyDeviceToHost));
        HIP_CHECK_RET(hipMemcpy(nr.data(), h->g.norms + r0 + s0, m * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < m; i++) {
            unsigned char *dst = out + (s0 + i) * fb;
            memcpy(dst, fr.data() + i * fw, fw);
            memcpy(dst + fw, &nr[i], 4);
            memset(dst + fw + 4, 0, fb - fw - 4);
        }
    }
    return LEANN_OK;
}
__global__ void bf16_to_f32_kernel(const uint16_t *__restrict__ in, size_t n, float *__restrict__ out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = __uint_as_float((uint32_t)in[i] << 16);
}

extern "C" int leann_recompute_build_index(const leann_recompute *r, int backend, size_t graph_degree, size_t complexity,
                                           leann_backend **out) {
    if (!r || !out) { leann_set_error("leann_recompute_build_index: null argument"); return LEANN_ERR_INVALID; }
    if (!r->parts.empty()) { leann_set_error("leann_recompute_build_index: build one index per part and join them with leann_sharded_from_handles"); return LEANN_ERR_UNSUPPORTED; }
    if (r->L != 1 || r->mask) {
        leann_set_error("recompute-on graph search needs one feature vector per passage (no token pooling): the feature-space "
                        "distance <f, W q> / ||W^T f|| is only exact for bf16-exact features");
        return LEANN_ERR_UNSUPPORTED;
    }
    HIP_CHECK_RET(hipSetDevice(r->device));
    const size_t n = r->n, ld = r->ld;
    DeviceBuf<float> E, norms; // (declared before the handle: it is closed first on an error return)
    DeviceBuf<unsigned char> rows_b;
    if (E.alloc(std::max<size_t>(n * ld, 4)) || norms.alloc(std::max<size_t>(n, 1))) return LEANN_ERR_DEVICE;
    int rc = LEANN_OK;
    for (size_t row0 = 0; row0 < n && rc == LEANN_OK; row0 += (size_t)4 << 20) { // transient embeddings, only for construction
        const size_t rows = std::min<size_t>((size_t)4 << 20, n - row0);
        rc = launch_encode(r, row0, rows, E + row0 * ld, nullptr, nullptr, 0, nullptr, norms + row0);
    }
    if (rc == LEANN_OK) HIP_CHECK_RET(hipDeviceSynchronize());
    leann_backend *built = nullptr;
    if (rc == LEANN_OK) rc = leann_backend_build_device(backend, E, n, r->d, ld, graph_degree, complexity, r->device, r->key_offset, 0, &built);
    if (rc != LEANN_OK) return rc;
    HandlePtr h(built); // borrows E until the swap below
    // swap the rows: features + inline norm replace the embeddings
    const uint32_t hp4 = (uint32_t)((r->h + 3) & ~(size_t)3);
    const bool split = hp4 == 256; // 512-B rows of whole lines + the norms in an array of their own (GraphView::norms)
    const uint32_t row_bytes = split ? 2 * hp4 : (2 * hp4 + 4 + 7) & ~7u;
    if (int e = rows_b.alloc(std::max<size_t>(n, 1) * row_bytes)) return e;
    HIP_CHECK_RET(hipMemset(rows_b, 0, std::max<size_t>(n, 1) * row_bytes));
    const uint64_t total = (uint64_t)n * (hp4 + 2);
    if (total)
        hipLaunchKernelGGL(pack_feature_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, nullptr, r->F, norms.p, (uint64_t)n,
                           (uint32_t)r->h, hp4, row_bytes, rows_b.p);
    if (int e = h->Wf32.alloc((size_t)hp4 * r->d)) return e;
    HIP_CHECK_RET(hipMemset(h->Wf32, 0, (size_t)hp4 * r->d * 4));
    hipLaunchKernelGGL(bf16_to_f32_kernel, dim3((unsigned)((r->h * r->d + 255) / 256)), dim3(256), 0, nullptr, r->Wraw, r->h * r->d, h->Wf32.p);
    HIP_CHECK_RET(hipGetLastError());
    HIP_CHECK_RET(hipDeviceSynchronize());
    E.reset();
    if (split) h->g.norms = h->store.norms = std::move(norms);
    leann_internal_own_rows(h.get(), std::move(rows_b));
    h->g.feat_h = hp4;
    h->g.row_bytes = row_bytes;
    *out = h.release();
    return LEANN_OK;
}

// raw feature rows [n x row_bytes] of a recompute-on index (tests: the oracle walks the same bytes)
extern "C" int leann_backend_feature_rows_export(const leann_backend *h, uint32_t *feat_h, uint32_t *row_bytes, void *out) {
    if (!h || !h->g.feat_h) { leann_set_error("not a recompute-on index"); return LEANN_ERR_INVALID; }
    if (feat_h) *feat_h = h->g.feat_h;
    if (row_bytes) *row_bytes = (uint32_t)leann_internal_feat_file_row_bytes(h->g); // the inline form, whatever the device layout
    if (out) return leann_internal_feat_rows_to_host(h, 0, (size_t)h->g.n, static_cast<unsigned char *>(out));
    return LEANN_OK;
}
