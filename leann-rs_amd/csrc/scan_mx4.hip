// scan_mx4.hip — MXFP4 rows: four bits per element and one E8M0 scale byte per 32 elements, searched exhaustively on the block-scaled
// matrix cores (include/leann_backend.h "MXFP4 rows"): leann_mx4_rows_*, leann_pack_mx4, leann_quantize_query_mx8 and
// the two search calls with their host-pointer twins.
//
// A row is KT = ceil(dims / 256) k-tiles: one 128-B line of E2M1 nibbles and 8 scale bytes per k-tile, codes and scales in two arrays
// whose layout IS the definition's.  The query gets E4M3 codes and its own block scales (MXFP8), the score is
// t_i = sum_blocks 2^(sx + sq - 254) sum_j A_j B_ij as v_mfma_scale_f32_32x32x64_f8f6f4 accumulates it in f32, the fetch_k best rows by
// t_i are the answer; the refined call hands them to leann_rerank_batch_device.
//
// Kernels:
//   pack_mx4_kernel              one wave per row and k-tile: lane l owns elements 4 l .. 4 l + 3, so a block is 8 lanes; its amax comes
//                                from three DPP steps (lane ^ 1, lane ^ 2, row_half_mirror), every lane packs its four nibbles into 16
//                                bits (the wave writes the 128-B line), the first lane of a block writes the scale byte.  Scale and
//                                codes are integer arithmetic on the f32 bits (mx4_scale, mx4_nibble below, which the host reference
//                                compiles too): no denormal mode, no rounding mode and no conversion instruction is relied on.
//   quantize_queries_mx8_kernel  one wave per query: finiteness over the whole query on the DPP ladder, then per k-tile the same
//                                8-lane amax, sq, four E4M3 codes per lane as one dword (mx8_code); Qc [nq rounded up to BQ x 256 KT],
//                                Qs [.. x 8 KT], padding queries zero, one "not finite" word per query.
//   score_mx4_mfma_kernel<LIST>  S[q][i] = t_i with A = the query's FP8 codes (cbsz = 0), B = the row's nibbles as they lie (blgp = 4,
//                                four VGPRs), both scales from registers.  A workgroup of 4 waves owns 128 rows x BQ queries, wave w the
//                                rows 32 w .. 32 w + 31 against all BQ queries; result layout and epilogue are score_i8_mfma_kernel's
//                                (slab S, or CandEmit against em.thr), so the select step of scan.hip is used unchanged.
//   mx4_no_answer_kernel         keys, scores and count of a query without codes (or of every query when no row is allowed): all tail.
//
// score_mx4_mfma_kernel, data movement.  A k-tile is 256 elements: ONE 128-B line of nibbles per row, TWO lines of FP8 per query, 8
// scale bytes of each.  Lane (l31, lh) of k-step s (four per k-tile, K = 64 each) supplies the scales of block 2 s + lh on both sides
// and the 16 B of its row's block 2 s + lh.  The FP8 operand is laid out differently (found on the device with unit vectors, then held
// by the tests): its lane (l31, lh) holds K = 16 lh .. 16 lh + 15 in VGPRs 0 - 3 and K = 32 + 16 lh .. in VGPRs 4 - 7, while the scale
// of K-block kb comes from the lanes with lh = kb for BOTH operands.  So the lane reads the 16-B columns lh and 2 + lh of the k-step's
// four query columns — half of block 2 s and half of block 2 s + 1 — and the scales stay as they are.  Thread t stages 16 B of row t / 8 (+ 32 per pass, 4 passes) at column t % 8 — a wave instruction reads eight whole
// lines — and 16 B of query t / 16 (+ 16 per pass, BQ / 16 passes) at column t % 16; threads 0 .. 127 stage the 8 scale bytes of row
// t, threads 128 .. 128 + BQ - 1 those of a query.  The next k-tile travels in registers while the current one is multiplied.  Rows
// and Qc are whole zero-padded k-tiles: no tail, no alignment branch.  With LIST, row i is idx[row0 + i], checked against n before it
// becomes an address; rows past the end of the launch are clamped to its last row and their scores never stored or emitted.
//
// LDS (static, no opt-in): sX [128][8] and sQ [64][16] of 16-B columns, 16 KiB each, sSx [128] and sSq [64] of 8 B: 34 304 B at
// BQ = 64 — four workgroups of a CU's 160 KiB, more than the registers allow.
//
// Scales.  A lane reads its row's 8 scale bytes as one ds_read_b64 and keeps the four of its k-half — blocks lh, 2 + lh, 4 + lh,
// 6 + lh — in ONE dword by a byte permute (v_perm_b32, selector 0x06040200 or 0x07050301); k-step s then picks byte s by opsel.  The
// same for each 32-query tile.  The scales are run-time register values everywhere (a literal 0 would let the backend select the
// unscaled instruction).
//
// Banks.  sX: column c of row r at slot c ^ sw(r), sw of score_i8_mfma_kernel, whose argument (scan_i8.hip) carries over unchanged: a
// half-wave's ds_read_b128 reads the SAME column of 32 consecutive rows 128 B apart, and sw spreads any aligned 8 (16) of them over
// all 32 (64) banks exactly once.  sQ: a query's line is 256 B, so column c of query q sits at slot c ^ (q & 15).  A half-wave reads
// one column of 32 consecutive queries, 256 B apart; over an aligned 8 of them (c ^ q) & 7 takes 8 values — the 32 banks of a 128-B
// clock once —, over an aligned 16 c ^ (q & 15) takes all 16 — the 64 banks of a 256-B clock once.  The staging write has 16
// consecutive lanes write the 16 slots of one query, a whole 256-B line.  The scale reads are 32 consecutive 8-B words, both halves
// of the wave the same ones (broadcast).  (Reasoned from the layout; the LDS conflict counter was not read.)
//
// Resource budget (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; nothing spills, no scratch instruction): see the table at
// MX4_BQ below.
#include "common.cuh"
#include "../../include/leann_backend.h"
#include "search.cuh"
#include "internal.h"
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
// Rows and queries of a workgroup's tile.  The resource report:
//   pack_mx4_kernel                        30 VGPRs,  0 AGPRs, LDS      0 B, 8 waves / SIMD
//   quantize_queries_mx8_kernel            16 VGPRs,  0 AGPRs, LDS      0 B, 8 waves / SIMD
//   mx4_no_answer_kernel                   10 VGPRs,  0 AGPRs, LDS      0 B, 8 waves / SIMD
//   score_mx4_mfma_kernel<false | true>   104 VGPRs, 32 AGPRs, LDS 34 304 B, 3 waves / SIMD            (BQ = 64)
//   the same at BQ = 128                  199 VGPRs, 64 AGPRs, LDS 51 200 B, 1 wave / SIMD, 48 spilled SGPRs
// BQ = 128 would halve the row bytes a batch above 64 queries streams through LDS but misses "two waves per SIMD, no spill", as it did
// for score_i8_mfma_kernel and score_bits_mfma_kernel: BQ = 64.  The compiled k-tile loop at BQ = 64 (read from the ISA listing) holds 8
// v_mfma_scale_f32_32x32x64_f8f6f4 with blgp:4 — the B operand in four VGPRs, op_sel and op_sel_hi running through the four scale
// bytes — and 3 v_perm_b32; nothing expands an operand on the vector ALU.
constexpr uint32_t MX4_BR = 128, MX4_BQ = 64;
constexpr size_t MX4_MAX_K = SEG / 2; // fetch_k: what the select step allows for k
constexpr size_t MX4_MAX_DIMS = 4096;

static inline size_t mx4_ktiles(size_t dims) { return (dims + 255) / 256; }
static inline size_t mx4_query_rows(size_t nq) { return (nq + MX4_BQ - 1) / MX4_BQ * MX4_BQ; }

// ---- the definition, steps 1-3, on the bits of an f32: host and device compile the same functions ------------------------------------
#define MX_FN __host__ __device__ __forceinline__
MX_FN uint32_t mx_bits(float x) { return __builtin_bit_cast(uint32_t, x); }
// |x| as bits, an element that is not finite as 0: non-negative floats order as their bits do, so the block's amax is an integer max
MX_FN uint32_t mx_abs_bits(uint32_t xb) {
    const uint32_t a = xb & 0x7FFFFFFFu;
    return a >= 0x7F800000u ? 0u : a;
}
MX_FN uint32_t mx4_scale(uint32_t amax_bits) { return (amax_bits >> 23) > 2u ? (amax_bits >> 23) - 2u : 0u; }
MX_FN uint32_t mx8_scale(uint32_t amax_bits) { return (amax_bits >> 23) > 8u ? (amax_bits >> 23) - 8u : 0u; }
// The nibble of x under the block scale sx.  |x| = m 2^(ex - 150), m the 24-bit significand and ex the exponent field (1 for a
// denormal), so |y| = |x| 2^(127 - sx) = m / 2^(u + 2) with u = 21 + sx - ex >= 19 (ex <= sx + 2): 0.25 is m == 2^u, and the table's
// thresholds are the multiples 1, 3, 5, 7, 10, 14, 20 of it — at most 20 * 2^23, inside 32 bits.  u >= 24 puts |y| below 0.25.
MX_FN uint32_t mx4_nibble(uint32_t xb, uint32_t sx) {
    const uint32_t a = xb & 0x7FFFFFFFu;
    if (a >= 0x7F800000u) return 0u;
    const uint32_t ex = a >> 23, m = (a & 0x7FFFFFu) | (ex ? 0x800000u : 0u), u = 21u + sx - (ex ? ex : 1u);
    uint32_t code = 0;
    if (u < 24u) {
        const uint32_t q = 1u << u;
        code = (m > q) + (m >= 3 * q) + (m > 5 * q) + (m >= 7 * q) + (m > 10 * q) + (m >= 14 * q) + (m > 20 * q);
    }
    return code | ((xb >> 31) << 3);
}
// The E4M3 code of a finite q under the block scale sq.  |y| = m / 2^sh, sh = 23 + sq - ex >= 15, below 512.  With p the top bit of m
// the unbiased exponent of |y| is e = p - sh <= 8; E4M3 rounds at a step of 2^(eb - 3), eb = max(e, -6) (-6: the subnormals, step
// 2^-9), so n = rne(m / 2^r), r = sh + eb - 3, is the significand in steps: 8 .. 16 for a normal, 0 .. 8 for a subnormal, and
// ((eb + 6) << 3) + n is the code in both cases, a carry (n = 16, or 8 for a subnormal) running into the exponent field as it should.
MX_FN uint32_t mx8_code(uint32_t qb, uint32_t sq) {
    const uint32_t a = qb & 0x7FFFFFFFu, sign = (qb >> 31) << 7;
    const uint32_t ex = a >> 23, m = (a & 0x7FFFFFu) | (ex ? 0x800000u : 0u);
    if (m == 0) return sign;
    const int sh = (int)(23u + sq - (ex ? ex : 1u)), e = 31 - __builtin_clz(m) - sh, eb = e < -6 ? -6 : e, r = sh + eb - 3;
    uint32_t n;
    if (r <= 0) n = m << -r; // r >= -3: exact
    else if (r > 25) n = 0;  // m < 2^24: below a quarter of a step
    else {
        const uint32_t rem = m & ((1u << r) - 1u), half = 1u << (r - 1);
        n = m >> r;
        n += (rem > half || (rem == half && (n & 1u))) ? 1u : 0u;
    }
    const uint32_t code = ((uint32_t)(eb + 6) << 3) + n;
    return sign | (code > 0x7Eu ? 0x7Eu : code); // 0x7E = 448; 0x7F is the NaN
}

// ---- the rows ---------------------------------------------------------------------------------------------------------------------------
// maximum over the aligned group of 8 lanes a lane belongs to, on ~v with the ladder's minimum; every lane gets the result
__device__ __forceinline__ uint32_t lanes8_max_u32(uint32_t v) {
    v = ~v;
    v = dpp_pair_min<0xB1, 0xf>(v);  // quad_perm [1,0,3,2]: lane ^ 1
    v = dpp_pair_min<0x4E, 0xf>(v);  // quad_perm [2,3,0,1]: lane ^ 2
    v = dpp_pair_min<0x141, 0xf>(v); // row_half_mirror: lane i of 8 <- lane 7 - i, the other quad
    return ~v;
}

// X [n x ld] f32 -> codes [n x 128 nkt], scales [n x 8 nkt]; one wave per row at a time, 4 rows per workgroup, grid-stride over the rows.
__global__ void __launch_bounds__(256) pack_mx4_kernel(const float *__restrict__ X, uint64_t n, uint32_t d, uint64_t ld, uint32_t nkt,
                                                       uint8_t *__restrict__ codes, uint8_t *__restrict__ scales) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t row = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += (uint64_t)gridDim.x * 4) {
        const float *x = X + row * ld;
        uint16_t *oc = reinterpret_cast<uint16_t *>(codes + row * 128 * nkt);
        uint8_t *os = scales + row * 8 * nkt;
        for (uint32_t kt = 0; kt < nkt; kt++) {
            const uint32_t j = 256 * kt + 4 * lane;
            uint32_t xb[4], mb = 0;
#pragma unroll
            for (uint32_t e = 0; e < 4; e++) {
                xb[e] = j + e < d ? __float_as_uint(x[j + e]) : 0u; // a padding column counts as +0: nibble 0, no sign
                mb = max(mb, mx_abs_bits(xb[e]));
            }
            const uint32_t sx = mx4_scale(lanes8_max_u32(mb));
            uint32_t w = 0;
#pragma unroll
            for (uint32_t e = 0; e < 4; e++) w |= mx4_nibble(xb[e], sx) << (4 * e);
            oc[64 * kt + lane] = (uint16_t)w;
            if ((lane & 7) == 0) os[8 * kt + (lane >> 3)] = (uint8_t)sx;
        }
    }
}

static int mx_check_pack(const char *who, bool null_in, const char *in_name, const void *codes, const void *scales, size_t dims) {
    if (null_in || !codes || !scales || dims < 1 || dims > MX4_MAX_DIMS) {
        leann_set_error("%s: %s%s", who, null_in || !codes || !scales ? "null " : "",
                        null_in ? in_name : !codes ? "codes_out" : !scales ? "scales_out" : "dims is outside [1, 4096]");
        return LEANN_ERR_INVALID;
    }
    return LEANN_OK;
}

extern "C" int leann_pack_mx4(const float *rows, size_t n, size_t dims, uint8_t *codes_out, uint8_t *scales_out) {
    if (int rc = mx_check_pack("leann_pack_mx4", n && !rows, "rows", codes_out, scales_out, dims)) return rc;
    const size_t nkt = mx4_ktiles(dims);
    memset(codes_out, 0, n * 128 * nkt);
    memset(scales_out, 0, n * 8 * nkt);
    for (size_t i = 0; i < n; i++)
        for (size_t b = 0; 32 * b < dims; b++) {
            const float *x = rows + i * dims;
            const size_t j1 = std::min(dims, 32 * b + 32);
            uint32_t mb = 0;
            for (size_t j = 32 * b; j < j1; j++) mb = std::max(mb, mx_abs_bits(mx_bits(x[j])));
            const uint32_t sx = mx4_scale(mb);
            scales_out[i * 8 * nkt + b] = (uint8_t)sx;
            for (size_t j = 32 * b; j < j1; j++) codes_out[i * 128 * nkt + (j >> 1)] |= (uint8_t)(mx4_nibble(mx_bits(x[j]), sx) << (4 * (j & 1)));
        }
    return LEANN_OK;
}

extern "C" int leann_quantize_query_mx8(const float *q, size_t dims, uint8_t *codes_out, uint8_t *scales_out) {
    if (int rc = mx_check_pack("leann_quantize_query_mx8", !q, "q", codes_out, scales_out, dims)) return rc;
    const size_t nkt = mx4_ktiles(dims);
    memset(codes_out, 0, 256 * nkt);
    memset(scales_out, 0, 8 * nkt);
    for (size_t j = 0; j < dims; j++)
        if ((mx_bits(q[j]) & 0x7FFFFFFFu) >= 0x7F800000u) { // no codes: every scale byte the E8M0 NaN
            memset(scales_out, 0xFF, 8 * nkt);
            return LEANN_OK;
        }
    for (size_t b = 0; 32 * b < dims; b++) {
        const size_t j1 = std::min(dims, 32 * b + 32);
        uint32_t mb = 0;
        for (size_t j = 32 * b; j < j1; j++) mb = std::max(mb, mx_bits(q[j]) & 0x7FFFFFFFu);
        const uint32_t sq = mx8_scale(mb);
        scales_out[b] = (uint8_t)sq;
        for (size_t j = 32 * b; j < j1; j++) codes_out[j] = (uint8_t)mx8_code(mx_bits(q[j]), sq);
    }
    return LEANN_OK;
}

struct leann_mx4_rows {
    size_t n = 0, dims = 0, nkt = 0;
    int device = 0;
    uint64_t key_offset = 0;
    DeviceBuf<uint8_t> codes, scales; // [n x 128 nkt], [n x 8 nkt]: the definition's layout
};

static int mx4_check_shape(const char *who, size_t n, size_t dims, int device, const void *out) {
    if (!out) { leann_set_error("%s: null out", who); return LEANN_ERR_INVALID; }
    if (dims < 1 || dims > MX4_MAX_DIMS) { leann_set_error("%s: dims = %zu is outside [1, 4096]", who, dims); return LEANN_ERR_INVALID; }
    if (n >= 0xFFFFFFFFull) { leann_set_error("%s: n = %zu is 2^32 - 1 or more", who, n); return LEANN_ERR_INVALID; }
    if (device < 0) { leann_set_error("%s: device = %d", who, device); return LEANN_ERR_INVALID; }
    return LEANN_OK;
}
static int mx4_new(size_t n, size_t dims, int device, uint64_t key_offset, std::unique_ptr<leann_mx4_rows> *out) {
    if (int rc = leann_internal_check_device(device)) return rc;
    HIP_CHECK_RET(hipSetDevice(device));
    std::unique_ptr<leann_mx4_rows> b(new leann_mx4_rows());
    b->n = n; b->dims = dims; b->nkt = mx4_ktiles(dims); b->device = device; b->key_offset = key_offset;
    if (int rc = b->codes.alloc(n * 128 * b->nkt)) return rc;
    if (int rc = b->scales.alloc(n * 8 * b->nkt)) return rc;
    *out = std::move(b);
    return LEANN_OK;
}
static int mx4_pack(leann_mx4_rows *b, const float *d_rows, size_t row0, size_t rows, size_t ld) {
    if (rows == 0) return LEANN_OK;
    const unsigned grid = (unsigned)std::min<size_t>((rows + 3) / 4, (size_t)1 << 20);
    hipLaunchKernelGGL(pack_mx4_kernel, dim3(grid), dim3(256), 0, nullptr, d_rows, (uint64_t)rows, (uint32_t)b->dims, (uint64_t)ld,
                       (uint32_t)b->nkt, b->codes.p + row0 * 128 * b->nkt, b->scales.p + row0 * 8 * b->nkt);
    HIP_CHECK_RET(hipGetLastError());
    HIP_CHECK_RET(hipStreamSynchronize(nullptr)); // the source rows are the caller's (or a slab that is filled again next)
    return LEANN_OK;
}

extern "C" int leann_mx4_rows_from_device(const float *d_rows, size_t n, size_t dims, size_t ld, int device, uint64_t key_offset,
                                          leann_mx4_rows **out) {
    const char *who = "leann_mx4_rows_from_device";
    if (out) *out = nullptr;
    if (int rc = mx4_check_shape(who, n, dims, device, out)) return rc;
    if (!d_rows && n) { leann_set_error("%s: null d_rows", who); return LEANN_ERR_INVALID; }
    if (ld < dims) { leann_set_error("%s: ld = %zu is below dims = %zu", who, ld, dims); return LEANN_ERR_INVALID; }
    std::unique_ptr<leann_mx4_rows> b;
    if (int rc = mx4_new(n, dims, device, key_offset, &b)) return rc;
    if (int rc = mx4_pack(b.get(), d_rows, 0, n, ld)) return rc;
    *out = b.release();
    return LEANN_OK;
}

extern "C" int leann_mx4_rows_from_host(const float *rows, size_t n, size_t dims, int device, uint64_t key_offset, leann_mx4_rows **out) {
    const char *who = "leann_mx4_rows_from_host";
    if (out) *out = nullptr;
    if (int rc = mx4_check_shape(who, n, dims, device, out)) return rc;
    if (!rows && n) { leann_set_error("%s: null rows", who); return LEANN_ERR_INVALID; }
    std::unique_ptr<leann_mx4_rows> b;
    if (int rc = mx4_new(n, dims, device, key_offset, &b)) return rc;
    // slabs of at most 256 MiB of f32 rows: the collection itself never has to fit beside its codes
    const size_t slab_rows = std::max<size_t>(1, std::min<size_t>(n, ((size_t)256 << 20) / (dims * 4)));
    DeviceBuf<float> slab;
    if (n)
        if (int rc = slab.alloc(slab_rows * dims)) return rc;
    for (size_t r0 = 0; r0 < n; r0 += slab_rows) {
        const size_t m = std::min(slab_rows, n - r0);
        HIP_CHECK_RET(hipMemcpy(slab, rows + r0 * dims, m * dims * 4, hipMemcpyHostToDevice));
        if (int rc = mx4_pack(b.get(), slab, r0, m, dims)) return rc;
    }
    *out = b.release();
    return LEANN_OK;
}

extern "C" size_t leann_mx4_rows_len(const leann_mx4_rows *b) { return b ? b->n : 0; }
extern "C" size_t leann_mx4_rows_dims(const leann_mx4_rows *b) { return b ? b->dims : 0; }
extern "C" size_t leann_mx4_rows_code_pitch(const leann_mx4_rows *b) { return b ? 128 * b->nkt : 0; }
extern "C" size_t leann_mx4_rows_scale_pitch(const leann_mx4_rows *b) { return b ? 8 * b->nkt : 0; }
extern "C" int leann_mx4_rows_export(const leann_mx4_rows *b, uint8_t *codes_out, uint8_t *scales_out) {
    if (!b || ((!codes_out || !scales_out) && b->n)) {
        leann_set_error("leann_mx4_rows_export: null %s", !b ? "mx4 rows" : !codes_out ? "codes_out" : "scales_out");
        return LEANN_ERR_INVALID;
    }
    if (b->n == 0) return LEANN_OK;
    HIP_CHECK_RET(hipSetDevice(b->device));
    HIP_CHECK_RET(hipMemcpy(codes_out, b->codes, b->n * 128 * b->nkt, hipMemcpyDeviceToHost));
    HIP_CHECK_RET(hipMemcpy(scales_out, b->scales, b->n * 8 * b->nkt, hipMemcpyDeviceToHost));
    return LEANN_OK;
}
extern "C" void leann_mx4_rows_close(leann_mx4_rows *b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    (void)hipDeviceSynchronize(); // no kernel still reads the codes
    delete b;
}

// ---- the query codes --------------------------------------------------------------------------------------------------------------------
// grid = nq rounded up to MX4_BQ; Qc [grid x 256 nkt], Qs [grid x 8 nkt].
__global__ void __launch_bounds__(64) quantize_queries_mx8_kernel(const float *__restrict__ Q, uint32_t nq, uint32_t d, uint32_t nkt,
                                                                  uint8_t *__restrict__ Qc, uint8_t *__restrict__ Qs,
                                                                  uint32_t *__restrict__ bad /* [nq] */) {
    const uint32_t q = blockIdx.x, lane = threadIdx.x;
    uint32_t *oc = reinterpret_cast<uint32_t *>(Qc + (size_t)q * 256 * nkt);
    uint8_t *os = Qs + (size_t)q * 8 * nkt;
    bool finite = false; // a padding query of the last tile: zero codes, scale 0
    const float *qv = Q + (size_t)q * d;
    if (q < nq) {
        uint32_t mb = 0; // bits of max |q_j|: a NaN or an infinity is >= 0x7F800000
        for (uint32_t j = lane; j < d; j += 64) mb = max(mb, __float_as_uint(qv[j]) & 0x7FFFFFFFu);
        finite = ~wave_min_u32(~mb) < 0x7F800000u;
        if (lane == 0) bad[q] = finite ? 0u : 1u;
    }
    for (uint32_t kt = 0; kt < nkt; kt++) {
        const uint32_t j = 256 * kt + 4 * lane;
        uint32_t qb[4], mb = 0;
#pragma unroll
        for (uint32_t e = 0; e < 4; e++) {
            qb[e] = finite && j + e < d ? __float_as_uint(qv[j + e]) : 0u;
            mb = max(mb, qb[e] & 0x7FFFFFFFu);
        }
        const uint32_t sq = mx8_scale(lanes8_max_u32(mb));
        uint32_t w = 0;
#pragma unroll
        for (uint32_t e = 0; e < 4; e++) w |= mx8_code(qb[e], sq) << (8 * e);
        oc[64 * kt + lane] = w;
        if ((lane & 7) == 0) os[8 * kt + (lane >> 3)] = (uint8_t)sq;
    }
}

// ---- the score --------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t mx4_sw(uint32_t r) { return ((r >> 1) & 7u) ^ ((r & 1u) << 2); } // sX's slot swizzle (scan_i8.hip)

// k-step S of the resident k-tile: block 2 S + lh of the wave's 32 rows against every 32-query tile; opsel S picks the block's scale
// byte.  The 8-bit operand's K order is not the 4-bit one's: of the k-step's 64 query bytes the lane's first four VGPRs are the 16-B
// column lh and its last four the column 2 + lh (see the file header).
template <int S, int QT>
__device__ __forceinline__ void mx4_kstep(const i32x4 *sX, const i32x4 *sQ, uint32_t xrow, uint32_t l31, uint32_t lh, uint32_t rsw,
                                          const uint32_t (&sa)[QT], uint32_t sb, f32x16 (&acc)[QT]) {
    const uint32_t blk = 2 * S + lh, qsw = l31 & 15u;
    const i32x4 b4 = sX[xrow * 8 + (blk ^ rsw)];
    const i32x8 b = {b4[0], b4[1], b4[2], b4[3], 0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < QT; t++) {
        const i32x4 lo = sQ[(32 * t + l31) * 16 + ((4 * S + lh) ^ qsw)], hi = sQ[(32 * t + l31) * 16 + ((4 * S + 2 + lh) ^ qsw)];
        const i32x8 a = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        acc[t] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc[t], 0 /* A: FP8 E4M3 */, 4 /* B: FP4 E2M1 */, S, (int)sa[t], S, (int)sb);
    }
}

// LIST: row i of the launch is store row idx[row0 + i] (the allowed positions, compacted ascending); scores, slab columns and emitted
// keys are then indexed by i, and finalize_scan_kernel (scan.hip) maps i -> idx[i].  Epilogue: score_mfma_kernel's contract.
template <bool LIST>
__global__ void __launch_bounds__(256) score_mx4_mfma_kernel(const uint8_t *__restrict__ Xc, const uint8_t *__restrict__ Xs, uint32_t nkt,
                                                             uint64_t n_store, const uint8_t *__restrict__ Qc, const uint8_t *__restrict__ Qs,
                                                             uint32_t nq, uint64_t row0, uint32_t n_rows,
                                                             float *__restrict__ S /* [nq x n_rows] */, CandEmit em,
                                                             const uint32_t *__restrict__ idx) {
    constexpr int QT = MX4_BQ / 32, QP = MX4_BQ / 16; // 32-query tiles of a wave; staging passes of the query tile
    __shared__ i32x4 sX[MX4_BR * 8];
    __shared__ i32x4 sQ[MX4_BQ * 16];
    __shared__ uint2 sSx[MX4_BR], sSq[MX4_BQ];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const uint32_t rbase = blockIdx.x * MX4_BR, qbase = blockIdx.y * MX4_BQ;
    f32x16 acc[QT];
#pragma unroll
    for (int t = 0; t < QT; t++)
#pragma unroll
        for (int i = 0; i < 16; i++) acc[t][i] = 0.f;
    auto store_row = [&](uint32_t r) { // checked before it becomes an address
        const uint32_t row = min(rbase + r, n_rows - 1);
        return min(LIST ? (uint64_t)idx[row0 + row] : row0 + row, n_store - 1);
    };
    const uint32_t sr = tid >> 3, sc = tid & 7;  // staging: row sr (+ 32 per pass), 16-B column sc
    const uint32_t qr = tid >> 4, qc = tid & 15; // staging: query qr (+ 16 per pass), 16-B column qc
    const uint8_t *xp[4], *qp[QP];
#pragma unroll
    for (int p = 0; p < 4; p++) xp[p] = Xc + store_row(sr + 32 * p) * 128 * nkt + 16 * sc;
#pragma unroll
    for (int p = 0; p < QP; p++) qp[p] = Qc + (size_t)(qbase + qr + 16 * p) * 256 * nkt + 16 * qc; // Qc and Qs are padded to the tile
    // the scale bytes: threads 0 .. 127 those of row tid, threads 128 .. 128 + BQ - 1 those of query tid - 128
    const bool srow_t = tid < MX4_BR, sq_t = tid >= MX4_BR && tid < MX4_BR + MX4_BQ;
    const uint8_t *sp = srow_t ? Xs + store_row(tid) * 8 * nkt : Qs + (size_t)(qbase + (sq_t ? tid - MX4_BR : 0)) * 8 * nkt;
    i32x4 xv[4], qv[QP];
    uint2 sv;
    auto gload = [&](uint32_t g) {
#pragma unroll
        for (int p = 0; p < 4; p++) xv[p] = *reinterpret_cast<const i32x4 *>(xp[p] + (size_t)g * 128);
#pragma unroll
        for (int p = 0; p < QP; p++) qv[p] = *reinterpret_cast<const i32x4 *>(qp[p] + (size_t)g * 256);
        sv = *reinterpret_cast<const uint2 *>(sp + (size_t)g * 8);
    };
    const uint32_t wslot = sc ^ mx4_sw(sr), qslot = qc ^ (qr & 15u); // (sw(sr + 32 p) == sw(sr), (qr + 16 p) & 15 == qr & 15)
    const uint32_t rsw = mx4_sw(l31), xrow = wave * 32 + l31;        // (sw(32 w + l31) == sw(l31))
    const uint32_t sel = lh ? 0x07050301u : 0x06040200u;             // the scale bytes of blocks lh, 2 + lh, 4 + lh, 6 + lh
    gload(0);
    for (uint32_t g = 0; g < nkt; g++) {
#pragma unroll
        for (int p = 0; p < 4; p++) sX[(sr + 32 * p) * 8 + wslot] = xv[p];
#pragma unroll
        for (int p = 0; p < QP; p++) sQ[(qr + 16 * p) * 16 + qslot] = qv[p];
        if (srow_t) sSx[tid] = sv;
        else if (sq_t) sSq[tid - MX4_BR] = sv;
        __syncthreads();
        if (g + 1 < nkt) gload(g + 1);
        const uint2 rs = sSx[xrow];
        const uint32_t sb = __builtin_amdgcn_perm(rs.y, rs.x, sel);
        uint32_t sa[QT];
#pragma unroll
        for (int t = 0; t < QT; t++) {
            const uint2 qs = sSq[32 * t + l31];
            sa[t] = __builtin_amdgcn_perm(qs.y, qs.x, sel);
        }
        mx4_kstep<0, QT>(sX, sQ, xrow, l31, lh, rsw, sa, sb, acc);
        mx4_kstep<1, QT>(sX, sQ, xrow, l31, lh, rsw, sa, sb, acc);
        mx4_kstep<2, QT>(sX, sQ, xrow, l31, lh, rsw, sa, sb, acc);
        mx4_kstep<3, QT>(sX, sQ, xrow, l31, lh, rsw, sa, sb, acc);
        __syncthreads();
    }
    // C/D layout: col = lane & 31 (row of X), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (query).
    const uint32_t row = rbase + xrow;
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
                        const float sv2 = acc[t][reg];
                        if (q < nq && sv2 >= em.thr[q]) {
                            const uint32_t slot = atomicAdd(&em.cnt[q], 1u);
                            if (slot < em.cap) em.list[(size_t)q * em.cap + slot] = ((uint64_t)(~f32_orderable(sv2)) << 32) | (uint32_t)pos;
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

static void launch_score_mx4(hipStream_t st, const leann_mx4_rows *b, const uint8_t *Qc, const uint8_t *Qs, size_t nq, size_t row0, size_t rows,
                             float *S, const CandEmit &em, const uint32_t *idx) {
    const dim3 grid((unsigned)((rows + MX4_BR - 1) / MX4_BR), (unsigned)((nq + MX4_BQ - 1) / MX4_BQ));
    if (idx)
        hipLaunchKernelGGL(score_mx4_mfma_kernel<true>, grid, dim3(256), 0, st, b->codes.p, b->scales.p, (uint32_t)b->nkt, (uint64_t)b->n, Qc, Qs,
                           (uint32_t)nq, (uint64_t)row0, (uint32_t)rows, S, em, idx);
    else
        hipLaunchKernelGGL(score_mx4_mfma_kernel<false>, grid, dim3(256), 0, st, b->codes.p, b->scales.p, (uint32_t)b->nkt, (uint64_t)b->n, Qc, Qs,
                           (uint32_t)nq, (uint64_t)row0, (uint32_t)rows, S, em, idx);
}

// grid = nq; a query without codes (bad[q], or every query when bad == null: no row is allowed) has count 0 and nothing but tail
__global__ void __launch_bounds__(64) mx4_no_answer_kernel(const uint32_t *__restrict__ bad, uint32_t k, uint64_t *__restrict__ keys,
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
// Follows bits_run (scan_bits.hip): plan, leases, begin, per chunk { score, select }, finish — which writes keys and scores straight
// into the caller's arrays —, once more on the slab schedule if a candidate list overflowed.  Returns with `st` synchronised.
static int mx4_run(const leann_mx4_rows *b, const float *d_queries, size_t nq, size_t fetch_k, const uint8_t *d_allow, uint64_t *d_keys,
                   float *d_scores, uint32_t *d_counts, hipStream_t st) {
    const uint32_t k = (uint32_t)fetch_k;
    const size_t nq_pad = mx4_query_rows(nq);
    // every return, early ones included, gives the scratch back — after the stream is idle (SyncFirst is declared last, so it runs first)
    ScratchLease<uint8_t> Qc, Qs;
    ScratchLease<uint32_t> bad, list;
    struct SyncFirst {
        hipStream_t st;
        ~SyncFirst() { (void)hipStreamSynchronize(st); }
    } sync_first{st};
    if (int e = Qc.acquire(nq_pad * 256 * b->nkt)) return e;
    if (int e = Qs.acquire(nq_pad * 8 * b->nkt)) return e;
    if (int e = bad.acquire(nq)) return e;
    hipLaunchKernelGGL(quantize_queries_mx8_kernel, dim3((unsigned)nq_pad), dim3(64), 0, st, d_queries, (uint32_t)nq, (uint32_t)b->dims,
                       (uint32_t)b->nkt, Qc.p, Qs.p, bad.p);
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
            launch_score_mx4(st, b, Qc, Qs, nq, p.chunks[c].first, p.chunks[c].second, S, run.chunk_emit(c), idx);
            rc = leann_internal_topk_select_chunk(run, c, 0, (uint32_t)nq);
        }
        bool overflowed = false;
        if (rc == LEANN_OK) rc = leann_internal_topk_finish(run, b->key_offset, idx, 0, d_keys, d_scores, d_counts, &overflowed);
        if (rc != LEANN_OK) return rc;
        if (!overflowed) break;
    }
    hipLaunchKernelGGL(mx4_no_answer_kernel, dim3((unsigned)nq), dim3(64), 0, st, m ? bad.p : nullptr, k, d_keys, d_scores, d_counts);
    HIP_CHECK_RET(hipGetLastError());
    HIP_CHECK_RET(hipStreamSynchronize(st));
    return LEANN_OK;
}

// what the entry points refuse, on the host, before any device work
static int mx4_check(const char *who, const leann_mx4_rows *b, const void *queries, size_t nq, size_t fetch_k, const void *keys,
                     const void *out2, const char *out2_name, const void *counts) {
    if (!b || (nq && (!queries || !keys || !out2 || !counts))) {
        leann_set_error("%s: null %s", who, !b ? "mx4 rows" : !queries ? "queries" : !keys ? "keys" : !out2 ? out2_name : "counts");
        return LEANN_ERR_INVALID;
    }
    if (fetch_k < 1 || fetch_k > MX4_MAX_K) { leann_set_error("%s: fetch_k = %zu is outside [1, %zu]", who, fetch_k, MX4_MAX_K); return LEANN_ERR_INVALID; }
    if (nq >= (1ull << 31)) { leann_set_error("%s: nq = %zu is 2^31 or more", who, nq); return LEANN_ERR_INVALID; }
    return LEANN_OK;
}
static int mx4_refined_check(const char *who, const leann_mx4_rows *b, const leann_exact_rows *r, const void *queries, size_t nq, size_t top_k,
                             size_t fetch_k, const void *keys, const void *dists, const void *counts) {
    if (!r) { leann_set_error("%s: null exact rows", who); return LEANN_ERR_INVALID; }
    if (int rc = mx4_check(who, b, queries, nq, fetch_k, keys, dists, "dists", counts)) return rc;
    if (top_k < 1) { leann_set_error("%s: top_k = 0", who); return LEANN_ERR_INVALID; }
    if (top_k > fetch_k) { leann_set_error("%s: top_k = %zu is above fetch_k = %zu", who, top_k, fetch_k); return LEANN_ERR_INVALID; }
    if (r->dims != b->dims) { leann_set_error("%s: the exact rows have dims = %zu, the mx4 rows %zu", who, r->dims, b->dims); return LEANN_ERR_INVALID; }
    if (r->device != b->device) {
        leann_set_error("%s: the exact rows are on device %d, the mx4 rows on device %d", who, r->device, b->device);
        return LEANN_ERR_INVALID;
    }
    if (r->key_offset > b->key_offset || b->key_offset + b->n > r->key_offset + r->n) {
        leann_set_error("%s: the exact rows cover positions [%llu, %llu), the mx4 rows need key_offset .. key_offset + len = [%llu, %llu)", who,
                        (unsigned long long)r->key_offset, (unsigned long long)(r->key_offset + r->n), (unsigned long long)b->key_offset,
                        (unsigned long long)(b->key_offset + b->n));
        return LEANN_ERR_INVALID;
    }
    return LEANN_OK;
}
// an empty object: every answer is empty
static int mx4_run_or_empty(const leann_mx4_rows *b, const float *d_queries, size_t nq, size_t fetch_k, const uint8_t *d_allow, uint64_t *d_keys,
                            float *d_scores, uint32_t *d_counts, hipStream_t st) {
    if (b->n) return mx4_run(b, d_queries, nq, fetch_k, d_allow, d_keys, d_scores, d_counts, st);
    hipLaunchKernelGGL(mx4_no_answer_kernel, dim3((unsigned)nq), dim3(64), 0, st, (const uint32_t *)nullptr, (uint32_t)fetch_k, d_keys, d_scores,
                       d_counts);
    HIP_CHECK_RET(hipGetLastError());
    HIP_CHECK_RET(hipStreamSynchronize(st));
    return LEANN_OK;
}

extern "C" int leann_mx4_rows_search_batch_device(const leann_mx4_rows *b, const float *d_queries, size_t nq, size_t fetch_k,
                                                  const uint8_t *d_allow, uint64_t *d_keys, float *d_scores, uint32_t *d_counts, void *stream) {
    if (int rc = mx4_check("leann_mx4_rows_search_batch_device", b, d_queries, nq, fetch_k, d_keys, d_scores, "scores", d_counts)) return rc;
    if (nq == 0) return LEANN_OK;
    HIP_CHECK_RET(hipSetDevice(b->device));
    return mx4_run_or_empty(b, d_queries, nq, fetch_k, d_allow, d_keys, d_scores, d_counts, (hipStream_t)stream);
}

// The candidates into library scratch, then the rerank on the same stream.
static int mx4_refined_run(const char *who, const leann_mx4_rows *b, const leann_exact_rows *r, const float *d_queries, size_t nq, size_t top_k,
                           size_t fetch_k, const uint8_t *d_allow, uint64_t *d_keys, float *d_dists, uint32_t *d_counts, hipStream_t st) {
    ScratchLease<uint64_t> w_keys;
    ScratchLease<float> w_scores;
    ScratchLease<uint32_t> w_counts;
    if (int e = w_keys.acquire(nq * fetch_k)) return e;
    if (int e = w_scores.acquire(nq * fetch_k)) return e;
    if (int e = w_counts.acquire(nq)) return e;
    int rc = mx4_run_or_empty(b, d_queries, nq, fetch_k, d_allow, w_keys, w_scores, w_counts, st);
    if (rc == LEANN_OK) rc = leann_rerank_batch_device(r, d_queries, nq, w_keys, w_counts, fetch_k, top_k, d_keys, d_dists, d_counts, nullptr, st);
    // the leases end with the call: nothing may still be reading the lists
    if (hipStreamSynchronize(st) != hipSuccess && rc == LEANN_OK) {
        leann_set_error("%s: the search or the rerank failed on the device", who);
        rc = LEANN_ERR_DEVICE;
    }
    return rc;
}

extern "C" int leann_mx4_rows_search_refined_batch_device(const leann_mx4_rows *b, const leann_exact_rows *r, const float *d_queries, size_t nq,
                                                          size_t top_k, size_t fetch_k, const uint8_t *d_allow, uint64_t *d_keys,
                                                          float *d_dists, uint32_t *d_counts, void *stream) {
    const char *who = "leann_mx4_rows_search_refined_batch_device";
    if (int rc = mx4_refined_check(who, b, r, d_queries, nq, top_k, fetch_k, d_keys, d_dists, d_counts)) return rc;
    if (nq == 0) return LEANN_OK;
    HIP_CHECK_RET(hipSetDevice(b->device));
    return mx4_refined_run(who, b, r, d_queries, nq, top_k, fetch_k, d_allow, d_keys, d_dists, d_counts, (hipStream_t)stream);
}

// the host-pointer twins: r == null is the plain search (k_out = fetch_k scores), else the refined one (k_out = top_k distances)
static int mx4_host_call(const char *who, const leann_mx4_rows *b, const leann_exact_rows *r, const float *queries, size_t nq, size_t top_k,
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
    if (int rc = r ? mx4_refined_run(who, b, r, d_q, nq, top_k, fetch_k, da, d_keys, d_out2, d_counts, nullptr)
                   : mx4_run_or_empty(b, d_q, nq, fetch_k, da, d_keys, d_out2, d_counts, nullptr))
        return rc;
    HIP_CHECK_RET(hipMemcpy(keys, d_keys, nq * k_out * 8, hipMemcpyDeviceToHost));
    HIP_CHECK_RET(hipMemcpy(out2, d_out2, nq * k_out * 4, hipMemcpyDeviceToHost));
    HIP_CHECK_RET(hipMemcpy(counts, d_counts, nq * 4, hipMemcpyDeviceToHost));
    return LEANN_OK;
}

extern "C" int leann_mx4_rows_search_batch(const leann_mx4_rows *b, const float *queries, size_t nq, size_t fetch_k, const uint8_t *allow,
                                           uint64_t *keys, float *scores, uint32_t *counts) {
    const char *who = "leann_mx4_rows_search_batch";
    if (int rc = mx4_check(who, b, queries, nq, fetch_k, keys, scores, "scores", counts)) return rc;
    return mx4_host_call(who, b, nullptr, queries, nq, 0, fetch_k, allow, keys, scores, counts);
}

extern "C" int leann_mx4_rows_search_refined_batch(const leann_mx4_rows *b, const leann_exact_rows *r, const float *queries, size_t nq,
                                                   size_t top_k, size_t fetch_k, const uint8_t *allow, uint64_t *keys, float *dists,
                                                   uint32_t *counts) {
    const char *who = "leann_mx4_rows_search_refined_batch";
    if (int rc = mx4_refined_check(who, b, r, queries, nq, top_k, fetch_k, keys, dists, counts)) return rc;
    return mx4_host_call(who, b, r, queries, nq, top_k, fetch_k, allow, keys, dists, counts);
}
