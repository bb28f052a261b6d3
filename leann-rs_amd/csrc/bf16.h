// bf16.h — the one f32 -> bf16 rounding of the library, for host and device code alike (recompute.hip's synthetic features, the bf16
// rounding kernel of rows_bf16.hip, leann_round_bf16).  Round to nearest even; a NaN stays a NaN (its quiet bit is set, so that a payload
// living in the low 16 bits alone cannot round to an infinity).  The widening back is exact: (uint32_t)b << 16.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LEANN_BF16_FN __host__ __device__ __forceinline__
#else
#define LEANN_BF16_FN static inline
#endif

LEANN_BF16_FN uint16_t f32_bits_to_bf16_rne(uint32_t u) {
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x40); // NaN stays NaN
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
LEANN_BF16_FN uint16_t f32_to_bf16_rne(float f) {
    uint32_t u;
#if defined(__HIP_DEVICE_COMPILE__)
    u = __float_as_uint(f);
#else
    memcpy(&u, &f, 4);
#endif
    return f32_bits_to_bf16_rne(u);
}
