"""The definition of PQ rows (include/leann_backend.h "PQ rows") restated in numpy: the reference of tests/test_cpu_pq_rows.py and
tests/test_gpu_pq_rows.py.  f32 steps are numpy f32 operations in the definition's order, float64 steps numpy float64."""
import numpy as np

NO_KEY = np.iinfo(np.uint64).max


def shape(dims, dsub):
    """(M, pitch)"""
    M = -(-dims // dsub)
    return M, 16 * -(-M // 16)


def sub(x, dsub, clean=True):
    """[.. x dims] -> [.. x M x dsub] f32: padding columns 0, and what is not finite 0 when `clean`"""
    x = np.asarray(x, np.float32)
    out = np.zeros(x.shape[:-1] + (shape(x.shape[-1], dsub)[0] * dsub,), np.float32)
    out[..., :x.shape[-1]] = np.where(np.isfinite(x), x, 0) if clean else x
    return out.reshape(x.shape[:-1] + (-1, dsub))


def codebooks(C, dims, dsub):
    """the caller's codebooks [M x 256 x dsub] with every column at or behind dims zero"""
    C = np.asarray(C, np.float32)
    cols = np.arange(len(C))[:, None] * dsub + np.arange(dsub)
    return np.where((cols < dims)[:, None, :], C, np.float32(0))


def encode(X, C, dsub):
    """step 1: codes uint8 [n x pitch]; the f32 difference form summed with j ascending, the first minimum"""
    X = np.asarray(X, np.float32)
    M, pitch = shape(X.shape[1], dsub)
    S, C, out = sub(X, dsub), codebooks(C, X.shape[1], dsub), np.zeros((len(X), pitch), np.uint8)
    with np.errstate(over="ignore"):
        for m in range(M):
            acc = np.zeros((len(X), 256), np.float32)
            for j in range(dsub):
                d = S[:, m, None, j] - C[m, None, :, j]
                acc = acc + d * d
            out[:, m] = acc.argmin(axis=1)
    return out


def query_lut(q, C, dsub):
    """step 2: (w int16 [M x 256], has_tables)"""
    q = np.asarray(q, np.float32)
    C, qs = codebooks(C, len(q), dsub), sub(q, dsub, clean=False)
    L64 = np.zeros(C.shape[:2])
    with np.errstate(all="ignore"):
        for j in range(dsub):
            L64 = L64 + qs[:, None, j].astype(np.float64) * C[:, :, j].astype(np.float64)
        L = L64.astype(np.float32)
    if not (np.isfinite(q).all() and np.isfinite(L).all()):
        return np.zeros(C.shape[:2], np.int16), False
    E = max(int(np.abs(L).max().view(np.uint32)) >> 23, 1)
    return np.rint(L.astype(np.float64) * 2.0 ** (140 - E)).astype(np.int16), True


def search(codes, Q, C, dsub, fetch_k, allow=None, key_offset=0):
    """steps 3 and 4 on codes [n x pitch]: (keys, scores, counts); the fetch_k allowed rows with the largest t = sum_m w[m][code],
    ties to the lower position; the tail is NO_KEY / -inf; a query without tables has count 0"""
    n, M = len(codes), shape(Q.shape[1], dsub)[0]
    pos = np.arange(n)
    if allow is not None:
        pos = pos[np.unpackbits(np.asarray(allow, np.uint8), bitorder="little")[:n].astype(bool)]
    keys = np.full((len(Q), fetch_k), NO_KEY, np.uint64)
    scores = np.full((len(Q), fetch_k), -np.inf, np.float32)
    counts = np.zeros(len(Q), np.uint32)
    for i, q in enumerate(Q):
        w, has = query_lut(q, C, dsub)
        if not has:
            continue
        t = w.astype(np.int32)[np.arange(M), codes[pos, :M]].sum(axis=1, dtype=np.int32)
        best = np.lexsort((pos, -t))[:fetch_k]
        m = counts[i] = len(best)
        keys[i, :m] = pos[best] + key_offset
        scores[i, :m] = t[best]
    return keys, scores, counts


def train(X, dsub, iters):
    """step 5: codebooks f32 [M x 256 x dsub]"""
    X = np.asarray(X, np.float32)
    S, M = sub(X, dsub), shape(X.shape[1], dsub)[0]
    C = S[np.arange(256) * len(X) // 256].transpose(1, 0, 2).copy()
    for _ in range(iters):
        code = encode(X, C, dsub)
        for m in range(M):
            for c in np.unique(code[:, m]):
                members = S[code[:, m] == c, m].astype(np.float64)
                C[m, c] = (members.cumsum(axis=0)[-1] / len(members)).astype(np.float32)  # summed in row order
    return C
