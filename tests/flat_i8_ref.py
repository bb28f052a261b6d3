"""Numpy restatement of the flat search on int8 rows (include/leann_backend.h "exhaustive search on int8 rows", steps 1-7), built on
tests/i8_ref.py and pyoracle.dist_canon, independent of csrc/i8_rows.h and csrc/scan_i8.hip."""
import numpy as np

import i8_ref
from refine_ref import NO_KEY, orderable

NONFINITE = -2 ** 31

def query_codes(q, e):
    """steps 1-4: (cq int8 [d] in element order, E); a q' that is not finite: zero codes and E = NONFINITE"""
    with np.errstate(over="ignore", invalid="ignore"):
        qs = np.ascontiguousarray(q, np.float32) * np.ldexp(np.float32(1), -e.astype(np.int32)).astype(np.float32)
    if not np.isfinite(qs).all():
        return np.zeros(len(qs), np.int8), NONFINITE
    amax = np.abs(qs).max()
    if amax == 0:
        return np.zeros(len(qs), np.int8), 0
    m, x = np.frexp(np.float64(amax))
    E = (7 if m <= 127.0 / 128.0 else 6) - int(x)
    scaled = np.ldexp(qs, E)  # exact scaling: float32 in, float32 out, no overflow whatever E is
    return np.clip(np.rint(scaled), -127, 127).astype(np.int8), E


class Index:
    """the int8 index over rows X: exponents, codes, widened rows"""

    def __init__(self, X):
        self.e, self.c = i8_ref.quantize(X)
        self.Xq = i8_ref.dequantize(self.c, self.e)
        self.c32 = self.c.astype(np.int32)

    def search(self, po, Q, top_k, fetch_k, allow=None, removed=(), key_offset=0):
        """steps 5-7 -> (keys [nq x top_k] u64, dists f32, counts u32); allow: bitmap (bits behind n ignored) or None"""
        n = len(self.c)
        ok = np.ones(n, bool) if allow is None else np.unpackbits(np.asarray(allow, np.uint8), bitorder="little")[:n].astype(bool)
        ok[list(removed)] = False
        pos = np.flatnonzero(ok)
        keys = np.full((len(Q), top_k), NO_KEY, np.uint64)
        dists = np.full((len(Q), top_k), np.inf, np.float32)
        counts = np.zeros(len(Q), np.uint32)
        for i, q in enumerate(np.ascontiguousarray(Q, np.float32)):
            cq, E = query_codes(q, self.e)
            if E == NONFINITE or not len(pos):
                continue
            s = self.c32[pos] @ cq.astype(np.int32)                        # exact: 127^2 * 4096 < 2^31
            cand = pos[np.argsort(-s.astype(np.float32), kind="stable")[:fetch_k]]  # RNE cast; ties -> the lower position
            d = np.array([po.dist_canon(q, self.Xq[j]) for j in cand], np.float32)
            order = np.lexsort((cand, orderable(d)))[:top_k]
            counts[i] = len(order)
            keys[i, :len(order)] = cand[order].astype(np.uint64) + np.uint64(key_offset)
            dists[i, :len(order)] = d[order]
        return keys, dists, counts
