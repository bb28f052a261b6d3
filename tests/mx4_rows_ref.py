"""The definition of MXFP4 rows (include/leann_backend.h "MXFP4 rows") restated in numpy, float64 throughout: where the library works
on the bits of an f32, this file multiplies by powers of two and compares values."""
import numpy as np

NO_KEY = np.iinfo(np.uint64).max
E2M1 = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6])


def ktiles(dims):
    return (dims + 255) // 256


def _blocks(x):
    """[m x dims] f32 -> (values padded with +0 to whole k-tiles, |values| with what is not finite as 0, exponent field of the block amax)"""
    x = np.atleast_2d(np.asarray(x, np.float32))
    P = np.zeros((len(x), 256 * ktiles(x.shape[1])), np.float32)
    P[:, :x.shape[1]] = x
    A = np.where(np.isfinite(P), np.abs(P), np.float32(0)).reshape(len(x), -1, 32)
    return P.reshape(A.shape), A, (A.max(axis=2).view(np.uint32) >> 23).astype(np.int64)


def pack(X):
    """steps 1 and 2: (codes [n x 128 KT], scales [n x 8 KT])"""
    P, A, E = _blocks(X)
    sx = np.maximum(E - 2, 0)
    y = A.astype(np.float64) * 2.0 ** (127 - sx)[:, :, None]
    mag = ((y > 0.25).astype(np.uint8) + (y >= 0.75) + (y > 1.25) + (y >= 1.75) + (y > 2.5) + (y >= 3.5) + (y > 5)).astype(np.uint8)
    nib = np.where(np.isfinite(P), mag | (np.signbit(P).astype(np.uint8) << 3), 0).astype(np.uint8).reshape(len(P), -1)
    return nib[:, 0::2] | (nib[:, 1::2] << 4), sx.astype(np.uint8)


def fp8_value(code):
    """OCP E4M3: bias 7, subnormal step 2^-9"""
    code = np.asarray(code, np.int64)
    e, m = (code >> 3) & 15, code & 7
    return np.where(code & 0x80, -1.0, 1.0) * np.where(e == 0, m * 2.0 ** -9, (8 + m) * 2.0 ** (e - 10))


def quantize_query(q):
    """step 3: (codes [256 KT], scales [8 KT], finite)"""
    P, A, E = _blocks(q)
    if not np.isfinite(P).all():
        return np.zeros(P.size, np.uint8), np.zeros(E.size, np.uint8), False
    sq = np.maximum(E - 8, 0)
    y = A.astype(np.float64) * 2.0 ** (127 - sq)[:, :, None]
    eb = np.maximum(np.where(y > 0, np.frexp(y)[1] - 1, -6), -6)  # floor(log2 y); the subnormals and 0 share -6
    n = np.rint(y * 2.0 ** (3 - eb)).astype(np.int64)             # the significand in steps of 2^(eb - 3), nearest even
    code = np.minimum(((eb + 6) << 3) + n, 0x7E)                  # a carry runs into the exponent field; above 448 -> 448
    return (code | (np.signbit(P).astype(np.int64) << 7)).astype(np.uint8).reshape(-1), sq.astype(np.uint8).reshape(-1), True


def terms(codes, scales, Q):
    """step 4 in float64 from the dequantised codes: (T [nq x n] scores, A [nq x n] sum_j |term_j|, finite [nq])"""
    nib = np.stack([codes & 15, codes >> 4], axis=2).reshape(len(codes), -1)
    R = np.where(nib & 8, -1.0, 1.0) * E2M1[nib & 7] * np.repeat(2.0 ** (scales.astype(np.int64) - 127), 32, axis=1)
    T, A, finite = np.zeros((len(Q), len(R))), np.zeros((len(Q), len(R))), np.zeros(len(Q), bool)
    for i, q in enumerate(np.asarray(Q, np.float32)):
        c, s, finite[i] = quantize_query(q)
        v = fp8_value(c) * np.repeat(2.0 ** (s.astype(np.int64) - 127), 32)
        T[i], A[i] = R @ v, np.abs(R) @ np.abs(v)
    return T, A, finite


def assert_order_free(A, g):
    """the precondition of exact equality: with g the granularity of every term, any f32 summation order is exact"""
    assert (A < 2.0 ** 24 * g).all(), A.max() / g


def allowed(n, allow):
    pos = np.arange(n)
    return pos if allow is None else pos[np.unpackbits(np.asarray(allow, np.uint8), bitorder="little")[:n].astype(bool)]


def search(T, finite, fetch_k, allow=None, key_offset=0):
    """step 5 on the scores T: the fetch_k allowed rows with the largest (float)t, ties to the lower position; tail NO_KEY / -inf"""
    pos = allowed(T.shape[1], allow)
    keys = np.full((len(T), fetch_k), NO_KEY, np.uint64)
    scores = np.full((len(T), fetch_k), -np.inf, np.float32)
    counts = np.zeros(len(T), np.uint32)
    for i in np.flatnonzero(finite):
        t = T[i, pos].astype(np.float32)
        best = np.lexsort((pos, -t))[:fetch_k]
        m = counts[i] = len(best)
        keys[i, :m] = pos[best] + key_offset
        scores[i, :m] = t[best]
    return keys, scores, counts
