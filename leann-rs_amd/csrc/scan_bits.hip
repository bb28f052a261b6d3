// scan_bits.hip — sign-bit rows: one bit per element, searched exhaustively on the integer matrix cores (include/leann_backend.h
// "sign-bit rows"): leann_bit_rows_*, leann_pack_sign_bits and the two search calls with their host-pointer twins.
//
// A row is b_ij = (x_ij > c_j), packed little-endian at a pitch of 16 ceil(dims / 128) bytes; the device store IS that layout.  The
// query gets the int8 flat search's codes with every column exponent 0 (i8_rows.h), the score is t_i = sum_j cq_j b_ij in int32, the
// fetch_k best rows by (float)t_i are the answer; the refined call hands them to leann_rerank_batch_device.
//
// Kernels:
//   pack_sign_bits_kernel        one wave per row and step: 64 consecutive elements, one coalesced 256-B read, one __ballot of x > c,
//                                the 64 bits written by lane 0 as one 8-byte vector store.  HBM-bound on the f32 read.
//   quantize_queries_bits_kernel one wave per query: amax on the DPP ladder, E, the codes into Qc [nq rounded up to BQ x 8 pitch],
//                                padding zero, in the order the expansion below produces, and one "not finite" word.
//   score_bits_mfma_kernel<LIST> S[q][i] = (float) sum_j cq_j b_ij with v_mfma_i32_32x32x32_i8, A = query codes, B = the row's bits
//                                expanded to 0/1 bytes IN REGISTERS.  A workgroup of 4 waves owns 128 rows x BQ queries, wave w the
//                                rows 32 w .. 32 w + 31 against all BQ queries; result layout and epilogue are score_i8_mfma_kernel's
//                                (slab S, or CandEmit against em.thr), so the select step of scan.hip is used unchanged.
//   bits_no_answer_kernel        keys, scores and count of a query without codes (or of every query when no row is allowed): all tail.
//
// score_bits_mfma_kernel, the bits.  A k-tile is 128 elements: 16 B of a row, four 32-bit words W0 .. W3.  Up to KC = 16 k-tiles of
// the tile's 128 rows (2 048 columns, 256 B per row, 32 KiB) are RESIDENT in LDS; wider rows take ceil(pitch / 256) such chunks, the
// accumulators running through.  (32 KiB, not the 64 KiB the widest row would want: with the 8 KiB of query codes three workgroups
// still share a CU's 160 KiB, and a static array needs no opt-in.)  Thread t stages 16 B of row t / 8 (+ 32 per pass) at k-tile t % 8
// (+ 8): eight lanes read one row's contiguous slice, and without LIST consecutive rows are consecutive in memory, so a wave
// instruction reads whole lines.  With LIST, row i is idx[row0 + i], checked against n before it becomes an address; rows past the
// end of the launch are clamped to its last row and their scores never stored or emitted.
//
// Expansion.  Lane (l31, lh) — row 32 w + l31, k-half lh — owns the words W(2 lh) and W(2 lh + 1) of its row's k-tile: ONE
// ds_read_b64 per k-tile.  Word u feeds the k-steps s = 2 u and 2 u + 1: the B operand of k-step 2 u + v is the four dwords
// (W >> (4 v + i)) & 0x01010101, i = 0 .. 3 — byte e of dword i is bit 8 e + i of W.  That is a shift and an AND per dword (the first
// dword of a word needs no shift): 15 vector ALU operations per two operands, against 24 for the nibble multiply
// (v * 0x00204081) & 0x01010101 of the natural order.  The price is paid once per query, not per row: an integer sum is order-free,
// so the query codes are WRITTEN in that order — byte 4 i + e of a 32-element group holds element 8 e + i — and lane (l31, lh) of
// k-step s reads the 16-B column 4 lh + s of its query's 128-B line.  The expanded operand is reused for every 32-query tile of the
// workgroup: 7.5 / QT vector operations per MFMA, QT = BQ / 32.
//
// Banks.  The 8-byte unit (k-tile kt, half lh, row r) sits at sB[(2 kt + lh) 128 + (r ^ 2 kt)]: transposed to [k-slice][row].  The XOR
// only permutes the rows of an aligned group of 32 (2 kt <= 30), so the 32 lanes of a half-wave — 32 consecutive rows, one k-slice —
// read 256 contiguous bytes, each 4-byte bank of a 128-B (or 256-B) LDS clock exactly once per clock: conflict-free, where a
// row-major [row][16 B] tile would put all 32 lanes on the same four banks.  The staging write has 16 consecutive lanes write rows
// r (even) and r + 1 at k-tiles 0 .. 7: units r ^ 2 kt and (r + 1) ^ 2 kt are the eight even and the eight odd offsets of one aligned
// group of 16 — one 128-B clock, no conflict (at 256 B per clock rows r + 2, r + 3 fall on the same sixteen units: two-way, on a
// write that happens once per 16 k-tiles).  The query codes go through sQ exactly as in score_i8_mfma_kernel (slot c ^ sw(r)); its
// bank argument (scan_i8.hip) carries over, a half-wave still reading ONE column of 32 consecutive queries.  (Reasoned from the
// layout; the LDS conflict counter was not read.)
//
// Bytes.  A workgroup reads 128 pitch bytes of rows and BQ * 8 pitch bytes of query codes (from L2): at BQ = 64 four times as many
// query bytes as row bytes stream through LDS.  What that costs is in profiles/bit_rows.md.
//
// Resource budget (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; nothing spills, no scratch instruction): see the table at
// BITS_BQ below.
#include "common.cuh"
#include "../../include/leann_backend.h"
#include "search.cuh"
#include "internal.h"
#include "i8_rows.h"
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
// Rows and queries of a workgroup's tile, k-tiles resident per chunk.  The resource report:
//   pack_sign_bits_kernel                  14 VGPRs,  0 AGPRs, LDS      0 B, 8 waves / SIMD
//   quantize_queries_bits_kernel           14 VGPRs,  0 AGPRs, LDS      0 B, 8 waves / SIMD
//   bits_no_answer_kernel                  10 VGPRs,  0 AGPRs, LDS      0 B, 8 waves / SIMD
//   score_bits_mfma_kernel<false | true>  102 VGPRs, 32 AGPRs, LDS 40 960 B, 3 waves / SIMD            (BQ = 64)
//   the same at BQ = 128                  199 VGPRs, 64 AGPRs, LDS 49 152 B, 1 wave / SIMD, 44 spilled SGPRs
// BQ = 128 would halve the expansion per MFMA but misses "two waves per SIMD, no spill", as it did for score_i8_mfma_kernel: BQ = 64.
// The compiled k-tile loop at BQ = 64 (read from the ISA listing): 8 MFMAs, 40 vector ALU instructions — 30 of the expansion (16
// v_and_b32, 14 v_lshrrev_b32) and 10 of address arithmetic —, one ds_read_b64 of bits, 8 ds_read_b128 and 2 ds_write_b128 of query
// codes, 2 global_load_dwordx4: 5 vector ALU instructions per MFMA.  Whether they hide under the MFMA issue: profiles/bit_rows.md.
constexpr uint32_t BITS_BR = 128, BITS_BQ = 64, BITS_KC = 16;
constexpr size_t BITS_MAX_K = SEG / 2; // fetch_k: what the select step allows for k
constexpr size_t BITS_MAX_DIMS = 4096;

static inline size_t bits_pitch(size_t dims) { return 16 * ((dims + 127) / 128); }
static inline size_t bits_query_rows(size_t nq) { return (nq + BITS_BQ - 1) / BITS_BQ * BITS_BQ; }

// ---- the rows ---------------------------------------------------------------------------------------------------------------------------
// X [n x ld] f32 -> out [n x pitch]; one wave per row at a time, 4 rows per workgroup, grid-stride over the rows.
__global__ void __launch_bounds__(256) pack_sign_bits_kernel(const float *__restrict__ X, uint64_t n, uint32_t d, uint64_t ld,
                                                             const float *__restrict__ center, uint32_t pitch,
                                                             uint8_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63, steps = pitch >> 3; // 64 bits per step; the padding bits of the last steps are written as zero
    for (uint64_t row = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += (uint64_t)gridDim.x * 4) {
        const float *x = X + row * ld;
        unsigned long long *o = reinterpret_cast<unsigned long long *>(out + row * pitch);
        for (uint32_t s = 0; s < steps; s++) {
            const uint32_t j = 64 * s + lane;
            bool bit = false;
            if (j < d) bit = x[j] > (center ? center[j] : 0.0f); // false for a NaN on either side, for equality and for -0 against +0
            const unsigned long long w = __ballot(bit);
            if (lane == 0) o[s] = w;
        }
    }
}

extern "C" int leann_pack_sign_bits(const float *rows, size_t n, size_t dims, const float *center, uint8_t *out) {
    if ((n && !rows) || !out || dims < 1 || dims > BITS_MAX_DIMS) {
        leann_set_error("leann_pack_sign_bits: %s", n && !rows ? "null rows" : !out ? "null out" : "dims is outside [1, 4096]");
        return LEANN_ERR_INVALID;
    }
    const size_t pitch = bits_pitch(dims);
    memset(out, 0, n * pitch);
    for (size_t i = 0; i < n; i++)
        for (size_t j = 0; j < dims; j++)
            if (rows[i * dims + j] > (center ? center[j] : 0.0f)) out[i * pitch + (j >> 3)] |= (uint8_t)(1u << (j & 7));
    return LEANN_OK;
}

struct leann_bit_rows {
    size_t n = 0, dims = 0, pitch = 0;
    int device = 0;
    uint64_t key_offset = 0;
    DeviceBuf<uint8_t> bits; // [n x pitch], the definition's layout
};

static int bits_check_shape(const char *who, size_t n, size_t dims, int device, const void *out) {
    if (!out) { leann_set_error("%s: null out", who); return LEANN_ERR_INVALID; }
    if (dims < 1 || dims > BITS_MAX_DIMS) { leann_set_error("%s: dims = %zu is outside [1, 4096]", who, dims); return LEANN_ERR_INVALID; }
    if (n >= 0xFFFFFFFFull) { leann_set_error("%s: n = %zu is 2^32 - 1 or more", who, n); return LEANN_ERR_INVALID; }
    if (device < 0) { leann_set_error("%s: device = %d", who, device); return LEANN_ERR_INVALID; }
    return LEANN_OK;
}
static int bits_new(size_t n, size_t dims, int device, uint64_t key_offset, std::unique_ptr<leann_bit_rows> *out) {
    if (int rc = leann_internal_check_device(device)) return rc;
    HIP_CHECK_RET(hipSetDevice(device));
    std::unique_ptr<leann_bit_rows> b(new leann_bit_rows());
    b->n = n; b->dims = dims; b->pitch = bits_pitch(dims); b->device = device; b->key_offset = key_offset;
    if (int rc = b->bits.alloc(n * b->pitch)) return rc;
    *out = std::move(b);
    return LEANN_OK;
}
static int bits_pack(leann_bit_rows *b, const float *d_rows, size_t row0, size_t rows, size_t ld, const float *d_center) {
    if (rows == 0) return LEANN_OK;
    const unsigned grid = (unsigned)std::min<size_t>((rows + 3) / 4, (size_t)1 << 20);
    hipLaunchKernelGGL(pack_sign_bits_kernel, dim3(grid), dim3(256), 0, nullptr, d_rows, (uint64_t)rows, (uint32_t)b->dims, (uint64_t)ld, d_center,
                       (uint32_t)b->pitch, b->bits.p + row0 * b->pitch);
    HIP_CHECK_RET(hipGetLastError());
    HIP_CHECK_RET(hipStreamSynchronize(nullptr)); // the source rows are the caller's (or a slab that is filled again next)
    return LEANN_OK;
}

extern "C" int leann_bit_rows_from_device(const float *d_rows, size_t n, size_t dims, size_t ld, const float *d_center, int device,
                                          uint64_t key_offset, leann_bit_rows **out) {
    const char *who = "leann_bit_rows_from_device";
    if (out) *out = nullptr;
    if (int rc = bits_check_shape(who, n, dims, device, out)) return rc;
    if (!d_rows && n) { leann_set_error("%s: null d_rows", who); return LEANN_ERR_INVALID; }
    if (ld < dims) { leann_set_error("%s: ld = %zu is below dims = %zu", who, ld, dims); return LEANN_ERR_INVALID; }
    std::unique_ptr<leann_bit_rows> b;
    if (int rc = bits_new(n, dims, device, key_offset, &b)) return rc;
    if (int rc = bits_pack(b.get(), d_rows, 0, n, ld, d_center)) return rc;
    *out = b.release();
    return LEANN_OK;
}

extern "C" int leann_bit_rows_from_host(const float *rows, size_t n, size_t dims, const float *center, int device, uint64_t key_offset,
                                        leann_bit_rows **out) {
    const char *who = "leann_bit_rows_from_host";
    if (out) *out = nullptr;
    if (int rc = bits_check_shape(who, n, dims, device, out)) return rc;
    if (!rows && n) { leann_set_error("%s: null rows", who); return LEANN_ERR_INVALID; }
    std::unique_ptr<leann_bit_rows> b;
    if (int rc = bits_new(n, dims, device, key_offset, &b)) return rc;
    // slabs of at most 256 MiB of f32 rows: the collection itself never has to fit beside its bits
    const size_t slab_rows = std::max<size_t>(1, std::min<size_t>(n, ((size_t)256 << 20) / (dims * 4)));
    DeviceBuf<float> slab, d_center;
    if (n)
        if (int rc = slab.alloc(slab_rows * dims)) return rc;
    if (center) {
        if (int rc = d_center.alloc(dims)) return rc;
        HIP_CHECK_RET(hipMemcpy(d_center, center, dims * 4, hipMemcpyHostToDevice));
    }
    for (size_t r0 = 0; r0 < n; r0 += slab_rows) {
        const size_t m = std::min(slab_rows, n - r0);
        HIP_CHECK_RET(hipMemcpy(slab, rows + r0 * dims, m * dims * 4, hipMemcpyHostToDevice));
        if (int rc = bits_pack(b.get(), slab, r0, m, dims, center ? d_center.p : nullptr)) return rc;
    }
    *out = b.release();
    return LEANN_OK;
}

extern "C" size_t leann_bit_rows_len(const leann_bit_rows *b) { return b ? b->n : 0; }
extern "C" size_t leann_bit_rows_dims(const leann_bit_rows *b) { return b ? b->dims : 0; }
extern "C" size_t leann_bit_rows_pitch(const leann_bit_rows *b) { return b ? b->pitch : 0; }
extern "C" int leann_bit_rows_export(const leann_bit_rows *b, uint8_t *out) {
    if (!b || (!out && b->n)) { leann_set_error("leann_bit_rows_export: null %s", !b ? "bit rows" : "out"); return LEANN_ERR_INVALID; }
    if (b->n == 0) return LEANN_OK;
    HIP_CHECK_RET(hipSetDevice(b->device));
    HIP_CHECK_RET(hipMemcpy(out, b->bits, b->n * b->pitch, hipMemcpyDeviceToHost));
    return LEANN_OK;
}
extern "C" void leann_bit_rows_close(leann_bit_rows *b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    (void)hipDeviceSynchronize(); // no kernel still reads the bits
    delete b;
}

// ---- the query codes --------------------------------------------------------------------------------------------------------------------
// grid = nq rounded up to BITS_BQ; Qc [grid x ldq], ldq = 8 pitch.  The int8 flat search's arithmetic (i8_rows.h) with scale 1.
__global__ void __launch_bounds__(64) quantize_queries_bits_kernel(const float *__restrict__ Q, uint32_t nq, uint32_t d, uint32_t ldq,
                                                                   int8_t *__restrict__ Qc, uint32_t *__restrict__ bad /* [nq] */) {
    const uint32_t q = blockIdx.x, lane = threadIdx.x;
    uint32_t *out = reinterpret_cast<uint32_t *>(Qc + (size_t)q * ldq);
    if (q >= nq) { // a padding query of the last tile
        for (uint32_t w = lane; w < (ldq >> 2); w += 64) out[w] = 0u;
        return;
    }
    const float *qv = Q + (size_t)q * d;
    uint32_t mb = 0; // bits of max |q_j|: non-negative floats order as their bits do, and a NaN or an infinity is >= 0x7F800000
    for (uint32_t j = lane; j < d; j += 64) mb = max(mb, __float_as_uint(qv[j]) & 0x7FFFFFFFu);
    mb = ~wave_min_u32(~mb);
    const float amax = __uint_as_float(mb);
    const bool finite = i8_query_finite(amax);
    const int E = finite ? i8_query_exponent(amax) : 0;
    // dword w = 8 g + i of the row: byte e is the code of element 32 g + 8 e + i (the order the score kernel's expansion produces)
    for (uint32_t w = lane; w < (ldq >> 2); w += 64) {
        const uint32_t j0 = (w & ~7u) * 4 + (w & 7u);
        uint32_t v = 0;
#pragma unroll
        for (uint32_t e = 0; e < 4; e++) {
            const uint32_t j = j0 + 8 * e;
            if (finite && j < d) v |= (uint32_t)(uint8_t)i8_query_code(qv[j], E) << (8 * e);
        }
        out[w] = v;
    }
    if (lane == 0) bad[q] = finite ? 0u : 1u;
}

// ---- the score --------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t bits_sw(uint32_t r) { return ((r >> 1) & 7u) ^ ((r & 1u) << 2); } // sQ's slot swizzle (scan_i8.hip)

// LIST: row i of the launch is store row idx[row0 + i] (the allowed positions, compacted ascending); scores, slab columns and emitted
// keys are then indexed by i, and finalize_scan_kernel (scan.hip) maps i -> idx[i].  Epilogue: score_mfma_kernel's contract.
template <bool LIST>
__global__ void __launch_bounds__(256) score_bits_mfma_kernel(const uint8_t *__restrict__ X, uint32_t pitch, uint64_t n_store,
                                                              const int8_t *__restrict__ Qc, uint32_t nq, uint64_t row0, uint32_t n_rows,
                                                              float *__restrict__ S /* [nq x n_rows] */, CandEmit em,
                                                              const uint32_t *__restrict__ idx) {
    constexpr int QT = BITS_BQ / 32; // 32-query tiles of a wave, and staging passes of the query tile
    __shared__ unsigned long long sB[BITS_KC * 2 * BITS_BR];
    __shared__ i32x4 sQ[BITS_BQ * 8];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const uint32_t rbase = blockIdx.x * BITS_BR, qbase = blockIdx.y * BITS_BQ;
    const uint32_t nkt = pitch >> 4, ldq = pitch << 3; // k-tiles of a row; bytes of a query's codes
    i32x16 acc[QT];
#pragma unroll
    for (int t = 0; t < QT; t++)
#pragma unroll
        for (int i = 0; i < 16; i++) acc[t][i] = 0;
    const uint32_t sr = tid >> 3, sc = tid & 7; // staging: row / query sr (+ 32 per pass), 16-B column sc (+ 8 for the bits' second half)
    const uint8_t *xp[4];
    const int8_t *qp[QT];
#pragma unroll
    for (int p = 0; p < 4; p++) {
        const uint32_t row = min(rbase + sr + 32 * p, n_rows - 1);
        const uint64_t srow = min(LIST ? (uint64_t)idx[row0 + row] : row0 + row, n_store - 1); // checked before it becomes an address
        xp[p] = X + srow * pitch + 16 * sc;
    }
#pragma unroll
    for (int p = 0; p < QT; p++) qp[p] = Qc + (size_t)(qbase + sr + 32 * p) * ldq + 16 * sc; // Qc is padded to the tile
    i32x4 qv[QT];
    auto gload = [&](uint32_t g) {
#pragma unroll
        for (int p = 0; p < QT; p++) qv[p] = *reinterpret_cast<const i32x4 *>(qp[p] + (size_t)g * 128);
    };
    const uint32_t wslot = sc ^ bits_sw(sr); // (sw(sr + 32 p) == sw(sr))
    const uint32_t rsw = bits_sw(l31);       // (sw(32 t + l31) == sw(l31))
    gload(0);
    for (uint32_t g = 0; g < nkt; g++) {
        const uint32_t kt = g & (BITS_KC - 1);
        if (kt == 0) { // the next chunk of bits becomes resident (the barrier that ended the last k-tile lets sB be overwritten)
            const uint32_t ktc = min(BITS_KC, nkt - g);
            i32x4 xv[2][4];
#pragma unroll
            for (int h = 0; h < 2; h++)
#pragma unroll
                for (int p = 0; p < 4; p++)
                    if (sc + 8 * h < ktc) xv[h][p] = *reinterpret_cast<const i32x4 *>(xp[p] + (size_t)(g + 8 * h) * 16);
#pragma unroll
            for (int h = 0; h < 2; h++)
#pragma unroll
                for (int p = 0; p < 4; p++)
                    if (sc + 8 * h < ktc) {
                        const uint32_t k2 = 2 * (sc + 8 * h), r = (sr + 32 * p) ^ k2;
                        sB[k2 * BITS_BR + r] = ((unsigned long long)(uint32_t)xv[h][p][1] << 32) | (uint32_t)xv[h][p][0];
                        sB[(k2 + 1) * BITS_BR + r] = ((unsigned long long)(uint32_t)xv[h][p][3] << 32) | (uint32_t)xv[h][p][2];
                    }
        }
#pragma unroll
        for (int p = 0; p < QT; p++) sQ[(sr + 32 * p) * 8 + wslot] = qv[p];
        __syncthreads();
        if (g + 1 < nkt) gload(g + 1);
        const unsigned long long bits = sB[(2 * kt + lh) * BITS_BR + ((wave * 32 + l31) ^ (2 * kt))];
#pragma unroll
        for (uint32_t s = 0; s < 4; s++) {
            const uint32_t W = (uint32_t)(bits >> (32 * (s >> 1))), sh = 4 * (s & 1);
            i32x4 b;
#pragma unroll
            for (uint32_t i = 0; i < 4; i++) b[i] = (int)((W >> (sh + i)) & 0x01010101u);
            const uint32_t slot = (4 * lh + s) ^ rsw;
#pragma unroll
            for (int t = 0; t < QT; t++) acc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(sQ[(32 * t + l31) * 8 + slot], b, acc[t], 0, 0, 0);
        }
        __syncthreads();
    }
    // C/D layout: col = lane & 31 (row of X), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (query).  (float)t is exact: |t| < 2^24.
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

static void launch_score_bits(hipStream_t st, const leann_bit_rows *b, const int8_t *Qc, size_t nq, size_t row0, size_t rows, float *S,
                              const CandEmit &em, const uint32_t *idx) {
    const dim3 grid((unsigned)((rows + BITS_BR - 1) / BITS_BR), (unsigned)((nq + BITS_BQ - 1) / BITS_BQ));
    if (idx)
        hipLaunchKernelGGL(score_bits_mfma_kernel<true>, grid, dim3(256), 0, st, b->bits.p, (uint32_t)b->pitch, (uint64_t)b->n, Qc, (uint32_t)nq,
                           (uint64_t)row0, (uint32_t)rows, S, em, idx);
    else
        hipLaunchKernelGGL(score_bits_mfma_kernel<false>, grid, dim3(256), 0, st, b->bits.p, (uint32_t)b->pitch, (uint64_t)b->n, Qc, (uint32_t)nq,
                           (uint64_t)row0, (uint32_t)rows, S, em, idx);
}

// grid = nq; a query without codes (bad[q], or every query when bad == null: no row is allowed) has count 0 and nothing but tail
__global__ void __launch_bounds__(64) bits_no_answer_kernel(const uint32_t *__restrict__ bad, uint32_t k, uint64_t *__restrict__ keys,
                                                            float *__restrict__ scores, uint32_t *__restrict__ counts) {
    const uint32_t q = blockIdx.x;
    if (bad && !bad[q]) return;
    for (uint32_t i = threadIdx.x; i < k; i += 64) {
        keys[(size_t)q * k + i] = ~0ull;
        scores[(size_t)q * k + i] = __uint_as_float(0xFF800000u); // -inf: the tail value of topk_finish's scores
    }
    if (threadIdx.x == 0) counts[q] = 0;
}

// ---- host side --------------------------------------------------------------------------------------------------------------------------
// Follows flat_i8_run (scan_i8.hip): plan, leases, begin, per chunk { score, select }, finish — which writes keys and scores straight
// into the caller's arrays —, once more on the slab schedule if a candidate list overflowed.  Returns with `st` synchronised.
static int bits_run(const leann_bit_rows *b, const float *d_queries, size_t nq, size_t fetch_k, const uint8_t *d_allow, uint64_t *d_keys,
                    float *d_scores, uint32_t *d_counts, hipStream_t st) {
    const uint32_t k = (uint32_t)fetch_k;
    const size_t nq_pad = bits_query_rows(nq), ldq = b->pitch * 8;
    // every return, early ones included, gives the scratch back — after the stream is idle (SyncFirst is declared last, so it runs first)
    ScratchLease<int8_t> Qc;
    ScratchLease<uint32_t> bad, list;
    struct SyncFirst {
        hipStream_t st;
        ~SyncFirst() { (void)hipStreamSynchronize(st); }
    } sync_first{st};
    if (int e = Qc.acquire(nq_pad * ldq)) return e;
    if (int e = bad.acquire(nq)) return e;
    hipLaunchKernelGGL(quantize_queries_bits_kernel, dim3((unsigned)nq_pad), dim3(64), 0, st, d_queries, (uint32_t)nq, (uint32_t)b->dims,
                       (uint32_t)ldq, Qc.p, bad.p);
    HIP_CHECK_RET(hipGetLastError());
    // the rows of the search: all of them, or the allowed ones as an ascending list
    size_t m = b->n;
    if (d_allow)
        if (int rc = leann_internal_compact_allow(d_allow, b->n, &list, &m, st)) return rc;
    const uint32_t *idx = d_allow ? list.p : nullptr;
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
            launch_score_bits(st, b, Qc, nq, p.chunks[c].first, p.chunks[c].second, S, run.chunk_emit(c), idx);
            rc = leann_internal_topk_select_chunk(run, c, 0, (uint32_t)nq);
        }
        bool overflowed = false;
        if (rc == LEANN_OK) rc = leann_internal_topk_finish(run, b->key_offset, idx, 0, d_keys, d_scores, d_counts, &overflowed);
        if (rc != LEANN_OK) return rc;
        if (!overflowed) break;
    }
    hipLaunchKernelGGL(bits_no_answer_kernel, dim3((unsigned)nq), dim3(64), 0, st, m ? bad.p : nullptr, k, d_keys, d_scores, d_counts);
    HIP_CHECK_RET(hipGetLastError());
    HIP_CHECK_RET(hipStreamSynchronize(st));
    return LEANN_OK;
}

// what the entry points refuse, on the host, before any device work
static int bits_check(const char *who, const leann_bit_rows *b, const void *queries, size_t nq, size_t fetch_k, const void *keys,
                      const void *out2, const char *out2_name, const void *counts) {
    if (!b || (nq && (!queries || !keys || !out2 || !counts))) {
        leann_set_error("%s: null %s", who, !b ? "bit rows" : !queries ? "queries" : !keys ? "keys" : !out2 ? out2_name : "counts");
        return LEANN_ERR_INVALID;
    }
    if (fetch_k < 1 || fetch_k > BITS_MAX_K) { leann_set_error("%s: fetch_k = %zu is outside [1, %zu]", who, fetch_k, BITS_MAX_K); return LEANN_ERR_INVALID; }
    if (nq >= (1ull << 31)) { leann_set_error("%s: nq = %zu is 2^31 or more", who, nq); return LEANN_ERR_INVALID; }
    return LEANN_OK;
}
static int bits_refined_check(const char *who, const leann_bit_rows *b, const leann_exact_rows *r, const void *queries, size_t nq, size_t top_k,
                              size_t fetch_k, const void *keys, const void *dists, const void *counts) {
    if (!r) { leann_set_error("%s: null exact rows", who); return LEANN_ERR_INVALID; }
    if (int rc = bits_check(who, b, queries, nq, fetch_k, keys, dists, "dists", counts)) return rc;
    if (top_k < 1) { leann_set_error("%s: top_k = 0", who); return LEANN_ERR_INVALID; }
    if (top_k > fetch_k) { leann_set_error("%s: top_k = %zu is above fetch_k = %zu", who, top_k, fetch_k); return LEANN_ERR_INVALID; }
    if (r->dims != b->dims) { leann_set_error("%s: the exact rows have dims = %zu, the bit rows %zu", who, r->dims, b->dims); return LEANN_ERR_INVALID; }
    if (r->device != b->device) {
        leann_set_error("%s: the exact rows are on device %d, the bit rows on device %d", who, r->device, b->device);
        return LEANN_ERR_INVALID;
    }
    if (r->key_offset > b->key_offset || b->key_offset + b->n > r->key_offset + r->n) {
        leann_set_error("%s: the exact rows cover positions [%llu, %llu), the bit rows need key_offset .. key_offset + len = [%llu, %llu)", who,
                        (unsigned long long)r->key_offset, (unsigned long long)(r->key_offset + r->n), (unsigned long long)b->key_offset,
                        (unsigned long long)(b->key_offset + b->n));
        return LEANN_ERR_INVALID;
    }
    return LEANN_OK;
}
// an empty object: every answer is empty
static int bits_run_or_empty(const leann_bit_rows *b, const float *d_queries, size_t nq, size_t fetch_k, const uint8_t *d_allow, uint64_t *d_keys,
                             float *d_scores, uint32_t *d_counts, hipStream_t st) {
    if (b->n) return bits_run(b, d_queries, nq, fetch_k, d_allow, d_keys, d_scores, d_counts, st);
    hipLaunchKernelGGL(bits_no_answer_kernel, dim3((unsigned)nq), dim3(64), 0, st, (const uint32_t *)nullptr, (uint32_t)fetch_k, d_keys, d_scores,
                       d_counts);
    HIP_CHECK_RET(hipGetLastError());
    HIP_CHECK_RET(hipStreamSynchronize(st));
    return LEANN_OK;
}

extern "C" int leann_bit_rows_search_batch_device(const leann_bit_rows *b, const float *d_queries, size_t nq, size_t fetch_k,
                                                  const uint8_t *d_allow, uint64_t *d_keys, float *d_scores, uint32_t *d_counts, void *stream) {
    if (int rc = bits_check("leann_bit_rows_search_batch_device", b, d_queries, nq, fetch_k, d_keys, d_scores, "scores", d_counts)) return rc;
    if (nq == 0) return LEANN_OK;
    HIP_CHECK_RET(hipSetDevice(b->device));
    return bits_run_or_empty(b, d_queries, nq, fetch_k, d_allow, d_keys, d_scores, d_counts, (hipStream_t)stream);
}

// The candidates into library scratch, then the rerank on the same stream.
static int bits_refined_run(const char *who, const leann_bit_rows *b, const leann_exact_rows *r, const float *d_queries, size_t nq, size_t top_k,
                            size_t fetch_k, const uint8_t *d_allow, uint64_t *d_keys, float *d_dists, uint32_t *d_counts, hipStream_t st) {
    ScratchLease<uint64_t> w_keys;
    ScratchLease<float> w_scores;
    ScratchLease<uint32_t> w_counts;
    if (int e = w_keys.acquire(nq * fetch_k)) return e;
    if (int e = w_scores.acquire(nq * fetch_k)) return e;
    if (int e = w_counts.acquire(nq)) return e;
    int rc = bits_run_or_empty(b, d_queries, nq, fetch_k, d_allow, w_keys, w_scores, w_counts, st);
    if (rc == LEANN_OK) rc = leann_rerank_batch_device(r, d_queries, nq, w_keys, w_counts, fetch_k, top_k, d_keys, d_dists, d_counts, nullptr, st);
    // the leases end with the call: nothing may still be reading the lists
    if (hipStreamSynchronize(st) != hipSuccess && rc == LEANN_OK) {
        leann_set_error("%s: the search or the rerank failed on the device", who);
        rc = LEANN_ERR_DEVICE;
    }
    return rc;
}

extern "C" int leann_bit_rows_search_refined_batch_device(const leann_bit_rows *b, const leann_exact_rows *r, const float *d_queries, size_t nq,
                                                          size_t top_k, size_t fetch_k, const uint8_t *d_allow, uint64_t *d_keys,
                                                          float *d_dists, uint32_t *d_counts, void *stream) {
    const char *who = "leann_bit_rows_search_refined_batch_device";
    if (int rc = bits_refined_check(who, b, r, d_queries, nq, top_k, fetch_k, d_keys, d_dists, d_counts)) return rc;
    if (nq == 0) return LEANN_OK;
    HIP_CHECK_RET(hipSetDevice(b->device));
    return bits_refined_run(who, b, r, d_queries, nq, top_k, fetch_k, d_allow, d_keys, d_dists, d_counts, (hipStream_t)stream);
}

// the host-pointer twins: r == null is the plain search (k_out = fetch_k scores), else the refined one (k_out = top_k distances)
static int bits_host_call(const char *who, const leann_bit_rows *b, const leann_exact_rows *r, const float *queries, size_t nq, size_t top_k,
                          size_t fetch_k, const uint8_t *allow, uint64_t *keys, float *out2, uint32_t *counts) {
    if (nq == 0) return LEANN_OK;
    HIP_CHECK_RET(hipSetDevice(b->device));
    const size_t k_out = r ? top_k : fetch_k;
    DeviceBuf<float> d_q, d_out2;
    DeviceBuf<uint64_t> d_keys;
    DeviceBuf<uint32_t> d_counts;
    DeviceBuf<uint8_t> d_allow;
    if (int rc = d_q.alloc(nq * b->dims)) return rc;
    if (int rc = d_keys.alloc(nq * k_out)) return rc;
    if (int rc = d_out2.alloc(nq * k_out)) return rc;
    if (int rc = d_counts.alloc(nq)) return rc;
    HIP_CHECK_RET(hipMemcpy(d_q, queries, nq * b->dims * 4, hipMemcpyHostToDevice));
    if (allow && b->n) {
        if (int rc = d_allow.alloc((b->n + 7) / 8)) return rc;
        HIP_CHECK_RET(hipMemcpy(d_allow, allow, (b->n + 7) / 8, hipMemcpyHostToDevice));
    }
    const uint8_t *da = allow && b->n ? d_allow.p : nullptr;
    if (int rc = r ? bits_refined_run(who, b, r, d_q, nq, top_k, fetch_k, da, d_keys, d_out2, d_counts, nullptr)
                   : bits_run_or_empty(b, d_q, nq, fetch_k, da, d_keys, d_out2, d_counts, nullptr))
        return rc;
    HIP_CHECK_RET(hipMemcpy(keys, d_keys, nq * k_out * 8, hipMemcpyDeviceToHost));
    HIP_CHECK_RET(hipMemcpy(out2, d_out2, nq * k_out * 4, hipMemcpyDeviceToHost));
    HIP_CHECK_RET(hipMemcpy(counts, d_counts, nq * 4, hipMemcpyDeviceToHost));
    return LEANN_OK;
}

extern "C" int leann_bit_rows_search_batch(const leann_bit_rows *b, const float *queries, size_t nq, size_t fetch_k, const uint8_t *allow,
                                           uint64_t *keys, float *scores, uint32_t *counts) {
    const char *who = "leann_bit_rows_search_batch";
    if (int rc = bits_check(who, b, queries, nq, fetch_k, keys, scores, "scores", counts)) return rc;
    return bits_host_call(who, b, nullptr, queries, nq, 0, fetch_k, allow, keys, scores, counts);
}

extern "C" int leann_bit_rows_search_refined_batch(const leann_bit_rows *b, const leann_exact_rows *r, const float *queries, size_t nq,
                                                   size_t top_k, size_t fetch_k, const uint8_t *allow, uint64_t *keys, float *dists,
                                                   uint32_t *counts) {
    const char *who = "leann_bit_rows_search_refined_batch";
    if (int rc = bits_refined_check(who, b, r, queries, nq, top_k, fetch_k, keys, dists, counts)) return rc;
    return bits_host_call(who, b, r, queries, nq, top_k, fetch_k, allow, keys, dists, counts);
}
