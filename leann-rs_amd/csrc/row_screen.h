// row_screen.h — the bound behind the split-plane row screen of the throughput beam search (search.cuh).
// Plain C++ on purpose: the device code and the stand-alone host test (host/row_screen_selftest.cpp) compile the same functions.
//
// A stored f32 row lives a second time as two planes of 16-bit halves: hi_i = the upper 16 bits of x_i (x_i truncated toward zero: a
// valid bf16), lo_i = the lower 16.  (hi_i << 16) | lo_i is x_i bit for bit.  The screen reads the hi plane alone and computes a number
// lb that is proved, below, to be <= the distance the canonical f32 chain (common.cuh) would compute for the row; a row whose lb
// is strictly above the distance of a full beam's last entry cannot enter that beam and its lo plane is never read.
//
// Notation: u = 2^-24 (unit round-off of f32, round to nearest), T = chunks of 256 elements per row (T <= 16), q the query in
// registers, x_i = hi_i + r_i.  Rows and queries are NOT assumed to have unit norm.
//
// (1) Truncation.  For a normal hi_i, r_i has the sign of hi_i and |r_i| < 2^-7 |hi_i| (hi_i keeps the leading one and seven more
//     bits; what is cut off is below one unit of its last place, 2^(e-7) <= 2^-7 |hi_i|).  If the exponent field of hi_i is zero
//     (hi_i is zero or subnormal) so is that of x_i, and |r_i| < 2^16 * 2^-149 = 2^-133.  With A* = sum |q_i hi_i|, S* = sum q_i hi_i
//     (exact) and Q = sum |q_i|:
//         P = sum q_i x_i  <=  S* + 2^-7 A* + 2^-133 Q       and       sum |q_i x_i|  <=  (1 + 2^-7) A* + 2^-133 Q.
// (2) The canonical chain: 256 accumulators, each a chain of T fmaf, then an 8-level pair tree; every result passes through at most
//     T + 8 roundings, so the canonical dot D satisfies  D <= P + g_c sum |q_i x_i|,  g_c = (1 + u)^(T+8) - 1 <= 24.1 u.
// (3) The screen's own sums.  Lane l accumulates s (of q_i hi_i) and a (of |q_i hi_i|) over its 4 T elements with the same 4 chains of T
//     fmaf and the same two in-lane additions: T + 2 roundings, g_1 = (1 + u)^(T+2) - 1 <= 18.1 u:
//         |s_l - S*_l| <= g_1 A*_l,      A*_l <= (1 + g_1') a_l  with  1 + g_1' = (1 - u)^-(T+2).
//     Then ONE value per lane, v_l = fmaf(C, a_l, s_l) (rs_lane_bound), and one canonical wave tree over the 64 v_l: U.
//         v_l >= s_l + C a_l - u (C a_l + |s_l|) >= s_l + (C - 1.02 u) a_l                       (|s_l| <= (1 + g_1)(1 + g_1') a_l)
//         U   >= sum v_l - ((1 + u)^6 - 1) sum |v_l| >= sum v_l - 6.2 u sum a_l                  (|v_l| <= 1.01 (1 + g_1)(1 + g_1') a_l)
//     Collecting the multiples of sum a_l that (1)-(3) need, with sum |q_i x_i| from (1):
//         2^-7 (1 + g_1')  +  g_1 (1 + g_1')  +  1.02 u  +  6.2 u  +  g_c (1 + 2^-7)(1 + g_1')   <   2^-7 + 51 u,
//     and C = 2^-7 + 2^-17 = 2^-7 + 128 u leaves 77 u sum a_l to spare:
//         D  <=  U - 77 u sum a_l + E_true,        E_true = (1 + g_c) 2^-133 Q + (underflow, below).
// (4) The last two operations.  V = fl(U + E) errs by at most u (|U| + E) <= 1.03 u sum a_l + u E, which the spare 77 u sum a_l and
//     E >= 2 E_true cover: V >= D as real numbers.  Rounding is monotone, so lb = fl(1 - V) <= fl(1 - D), and fl(1 - D) IS the
//     distance of the kept path — the rounding of `1 - dot` needs no term of its own.
// (5) Underflow.  An fmaf whose result is subnormal errs by at most 2^-150 more than (2)-(3) count (additions are exact there); were
//     subnormals flushed instead, an operation or an operand loses at most 2^-126 (times |q_i| for an operand).  Fewer than 2^14
//     operations per row in either chain: below 2^-112 + 2^-126 Q.  rs_abs_term returns E = 2^-100 + 2^-119 Q', Q' the f32 sum of |q_i|
//     (its own rounding, relative 24.1 u, vanishes in the factor 2^7 between 2^-119 and 2 (2^-126 + 2^-133 (1 + g_c))).
// A NaN or an infinity anywhere makes lb NaN or -inf, `lb > worst` false, and the row takes the full path.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LEANN_RS_FN __host__ __device__ __forceinline__
#else
#define LEANN_RS_FN static inline
#endif

#define LEANN_RS_C 0x1.004p-7f /* 2^-7 + 2^-17 */

LEANN_RS_FN float rs_bits_to_f32(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
LEANN_RS_FN uint32_t rs_f32_to_bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
// the two planes of one element, and back
LEANN_RS_FN uint16_t rs_hi16(float x) { return (uint16_t)(rs_f32_to_bits(x) >> 16); }
LEANN_RS_FN uint16_t rs_lo16(float x) { return (uint16_t)(rs_f32_to_bits(x) & 0xFFFFu); }
LEANN_RS_FN float rs_join(uint16_t hi, uint16_t lo) { return rs_bits_to_f32(((uint32_t)hi << 16) | lo); }

// (3): one lane's share of the upper bound on the dot product, from its sums s of q_i hi_i and a of |q_i hi_i|
LEANN_RS_FN float rs_lane_bound(float s, float a) { return fmaf(LEANN_RS_C, a, s); }
// (5): the absolute term, from the f32 sum of |q_i| (once per query)
LEANN_RS_FN float rs_abs_term(float qabs) { return fmaf(qabs, 0x1p-119f, 0x1p-100f); }
// (4): lower bound on the canonical distance 1 - dot, from the wave-tree sum U of the lanes' bounds
LEANN_RS_FN float rs_lower_bound(float U, float E) { return 1.0f - (U + E); }

// Where element j of a row sits in its plane row of ldp u16 (ldp: ld rounded up to 64 elements, so a plane row is whole 128-B lines).
// Whole 512-element blocks are interleaved so that lane l (elements 256 t + 4 l .. + 3 of chunks t = 2 p and 2 p + 1) finds its eight
// halves of the block in ONE 16-byte load: position 512 p + 8 l + 4 (t & 1) + e.  The tail (< 512 elements) stays in element order:
// 8 bytes per lane and chunk.  Every fetched line is used in full either way.
LEANN_RS_FN uint32_t rs_plane_pos(uint32_t j, uint32_t ldp) {
    const uint32_t blk = j >> 9;
    if (((blk + 1) << 9) > ldp) return j;
    const uint32_t w = j & 511u, t = w >> 8, l = (w & 255u) >> 2, e = w & 3u;
    return (blk << 9) + 8u * l + 4u * t + e;
}
