"""The definition of sign-bit rows (include/leann_backend.h "sign-bit rows") restated in numpy: the reference of tests/test_cpu_bit_rows.py
and tests/test_gpu_bit_rows.py.  The query codes are the library's own host quantiser leann_quantize_query_i8 with every exponent 0,
as the definition says; everything else is integer arithmetic here."""
import numpy as np

NO_KEY = np.iinfo(np.uint64).max


def pitch(dims):
    return 16 * ((dims + 127) // 128)


def pack(X, center=None):
    """b_ij = x_ij > c_j (false for a NaN on either side), little-endian bits, rows padded with zero bits to the pitch"""
    X = np.asarray(X, np.float32)
    bits = X > (np.float32(0) if center is None else np.asarray(center, np.float32))
    out = np.zeros((len(X), pitch(X.shape[1])), np.uint8)
    packed = np.packbits(bits, axis=1, bitorder="little")
    out[:, :packed.shape[1]] = packed
    return out


def search(la, B, dims, Q, fetch_k, allow=None, key_offset=0):
    """packed rows B [n x pitch] -> (keys, scores, counts): the fetch_k allowed rows with the largest t = sum_j cq_j b_j, ties to the
    lower position; the tail is NO_KEY / -inf; a query without codes has count 0"""
    n = len(B)
    bits = np.unpackbits(B, axis=1, bitorder="little")[:, :dims].astype(np.int32)
    pos = np.arange(n)
    if allow is not None:
        pos = pos[np.unpackbits(np.asarray(allow, np.uint8), bitorder="little")[:n].astype(bool)]
    keys = np.full((len(Q), fetch_k), NO_KEY, np.uint64)
    scores = np.full((len(Q), fetch_k), -np.inf, np.float32)
    counts = np.zeros(len(Q), np.uint32)
    for i, q in enumerate(np.asarray(Q, np.float32)):
        codes, E = la.quantize_query_i8(q, np.zeros(dims, np.int8))
        if E == -2 ** 31:
            continue
        t = bits[pos] @ codes.astype(np.int32)
        best = np.lexsort((pos, -t))[:fetch_k]
        m = counts[i] = len(best)
        keys[i, :m] = pos[best] + key_offset
        scores[i, :m] = t[best]
    return keys, scores, counts
