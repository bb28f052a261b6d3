"""int8 rows in numpy, for the tests of the int8 row type (include/leann_backend.h "row types"), restated independently of
csrc/i8_rows.h: for rows X [n x d], all finite,
    amax_j = max_i |x_ij|;  e_j = the largest integer in [-32, 32] with amax_j 2^e_j <= 127 (0 when amax_j == 0);
    c_ij = clamp(rne(x_ij 2^e_j), -127, 127), the product taken in f32;  Xq_ij = (float)c_ij 2^-e_j (exact)."""
import numpy as np


def exponents(x):
    """e: int8 [d]"""
    amax = np.abs(np.ascontiguousarray(x, np.float32)).max(axis=0) if len(x) else np.zeros(np.shape(x)[1], np.float32)
    m, p = np.frexp(amax.astype(np.float64))  # amax = m 2^p, m in [0.5, 1): m 2^(p + e) <= 127 = (127 / 128) 2^7
    e = np.where(m <= 127.0 / 128.0, 7, 6) - p
    return np.where(amax == 0, 0, np.clip(e, -32, 32)).astype(np.int8)


def codes(x, e):
    """c: int8 [n x d]; np.rint rounds half to even, and float32 x float32 stays float32"""
    x = np.ascontiguousarray(x, np.float32)
    scaled = x * np.ldexp(np.float32(1), e.astype(np.int32)).astype(np.float32)[None, :]
    assert scaled.dtype == np.float32
    return np.clip(np.rint(scaled), -127, 127).astype(np.int8)


def dequantize(c, e):
    """Xq: float32 [n x d], exact"""
    return c.astype(np.float32) * np.ldexp(np.float32(1), -e.astype(np.int32)).astype(np.float32)[None, :]


def quantize(x):
    """(e, c)"""
    e = exponents(x)
    return e, codes(x, e)


def dequantized(x):
    """Xq of X"""
    e, c = quantize(x)
    return dequantize(c, e)
