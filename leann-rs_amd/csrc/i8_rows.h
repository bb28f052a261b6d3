// i8_rows.h — the definition of int8 rows (LEANN_ROWS_I8; include/leann_backend.h "row types", DESIGN.md "int8 rows") in plain C++: the
// device code (rows_i8.hip, search.cuh), the host quantiser (leann_quantize_i8) and the file checks compile the same functions.
//
// For rows X [n x d], all finite:  amax_j = max_i |x_ij|;  e_j = the largest integer in [-32, 32] with amax_j 2^e_j <= 127 (0 when
// amax_j == 0);  c_ij = clamp(rne(x_ij 2^e_j), -127, 127), the product taken in f32;  Xq_ij = (float)c_ij 2^-e_j (exact).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LEANN_I8_FN __host__ __device__ __forceinline__
#else
#define LEANN_I8_FN static inline
#endif

#define LEANN_I8_EXP_MAX 32

// e_j from amax_j (finite, >= 0).  amax = m 2^x with m in [0.5, 1): m 2^(x + e) <= 127 = (127 / 128) 2^7  <=>  e <= 7 - x when
// m <= 127 / 128, else e <= 6 - x.
LEANN_I8_FN int i8_exponent(float amax) {
    if (!(amax > 0.f)) return 0;
    int x;
    const float m = frexpf(amax, &x);
    const int e = (m <= 0.9921875f ? 7 : 6) - x;
    return e > LEANN_I8_EXP_MAX ? LEANN_I8_EXP_MAX : e < -LEANN_I8_EXP_MAX ? -LEANN_I8_EXP_MAX : e;
}
// 2^e for |e| <= 32: exact
LEANN_I8_FN float i8_pow2(int e) { return ldexpf(1.0f, e); }
// c = clamp(rne(x 2^e), -127, 127); `scale` = 2^e.  (rintf under the default rounding mode: to nearest, ties to even.)
LEANN_I8_FN int8_t i8_code(float x, float scale) {
    const float r = rintf(x * scale);
    return (int8_t)(r > 127.f ? 127.f : r < -127.f ? -127.f : r);
}

// The store's pitch: dims rounded up to 128 — a row is whole, aligned 128-B lines.
LEANN_I8_FN uint32_t i8_store_ld(uint32_t d) { return (d + 127u) & ~127u; }
// Where element j of a row sits in its store row of ldb bytes.  Whole 1 024-element blocks are interleaved so that lane l (elements
// 256 t + 4 l .. + 3 of the block's four chunks t) finds its sixteen codes in ONE 16-byte load: position 1024 b + 16 l + 4 t + e.  Of the
// tail (< 1 024 elements) a leading 512-element pair is interleaved the same way for one 8-byte load (512 p + 8 l + 4 t + e); the rest
// stays in element order: 4 bytes per lane and chunk.  Every fetched line is used in full either way.
LEANN_I8_FN uint32_t i8_row_pos(uint32_t j, uint32_t ldb) {
    const uint32_t base = j & ~1023u, w = j & 1023u, t = w >> 8, l = (w & 255u) >> 2, e = w & 3u;
    if (base + 1024u <= ldb) return base + 16u * l + 4u * t + e;
    if (w < 512u && base + 512u <= ldb) return base + 8u * l + 4u * t + e;
    return j;
}
