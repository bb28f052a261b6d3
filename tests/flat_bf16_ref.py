"""Numpy restatement of the flat search on bf16 rows (include/leann_backend.h "exhaustive search on bf16 rows"), built on
tests/bf16_ref.py and pyoracle.dist_canon, independent of csrc/scan_bf16.hip.

Pieces: hi = r(q), lo = r(q - w(hi)), the subtraction exact in f32; a query with a w(hi_j) that is not finite has none (count 0).
Screen: s_i = sum_j (w(hi_j) + w(lo_j)) w(x_ij), here in float64 — the device sums in f32 in an order the definition leaves open, so a
test compares with the screened answer only on inputs whose sums are exact in every order, else with the exact one behind its gap.
Candidates: the fetch_k largest s among the live allowed rows, ties to the lower position.  Answer: d = po.dist_canon(q, w(x_i)),
sorted by (d, position), the first top_k; keys = position + key_offset, the tail UINT64_MAX / +inf."""
import numpy as np

from bf16_ref import round_bf16, rounded, widen
from refine_ref import NO_KEY, orderable


def split(q):
    q = np.ascontiguousarray(q, np.float32)
    hi = round_bf16(q)
    with np.errstate(invalid="ignore"):
        return hi, round_bf16(q - widen(hi))


class Index:
    def __init__(self, X):
        self.Xr = rounded(X)
        self.X64, self.ldb = self.Xr.astype(np.float64), (X.shape[1] + 63) // 64 * 64

    def search(self, po, Q, top_k, fetch_k, key_offset=0, allow=None, removed=(), exact=False):
        """-> ((keys, dists, counts), gap).  exact: no screen — the exact top_k by (canonical distance, position) over the live allowed
        rows, and gap = the least distance, over the queries, between the canonical distances at ranks top_k and fetch_k + 1, in units
        of eps = 4 ldb 2^-23 max|q| max|x|: a worst-case bound on screen plus canonical rounding for any summation order, truncating
        accumulation included.  gap > 1: no screen within the bound can lose an answer.  (Rows whose float64 dot lies more than 2 eps
        below the (fetch_k + 1)-th largest cannot be among the first fetch_k + 1 and are not scored.)"""
        n, Q = len(self.Xr), np.ascontiguousarray(Q, np.float32)
        ok = np.ones(n, bool) if allow is None else np.unpackbits(np.asarray(allow, np.uint8), bitorder="little")[:n].astype(bool)
        ok[list(removed)] = False
        pos, gap = np.flatnonzero(ok), np.inf
        eps = 4 * self.ldb * 2.0 ** -23 * np.linalg.norm(Q.astype(np.float64), axis=1).max() * np.linalg.norm(self.X64, axis=1).max()
        keys = np.full((len(Q), top_k), NO_KEY, np.uint64)
        dists = np.full((len(Q), top_k), np.inf, np.float32)
        counts = np.zeros(len(Q), np.uint32)
        for i, q in enumerate(Q):
            hi, lo = split(q)
            if not np.isfinite(widen(hi)).all() or not len(pos):
                continue
            if exact:
                s = self.X64[pos] @ q.astype(np.float64)
                cand = pos[s >= np.sort(s)[::-1][min(fetch_k + 1, len(s)) - 1] - 2 * eps]
            else:
                s = self.X64[pos] @ (widen(hi).astype(np.float64) + widen(lo).astype(np.float64))
                cand = pos[np.argsort(-s, kind="stable")[:fetch_k]]
            d = np.array([po.dist_canon(q, self.Xr[j]) for j in cand], np.float32)
            o = np.lexsort((cand, orderable(d)))
            if exact and len(o) > fetch_k:
                gap = min(gap, (float(d[o[fetch_k]]) - float(d[o[top_k - 1]])) / eps)
            o = o[:top_k]
            counts[i] = len(o)
            keys[i, :len(o)] = cand[o].astype(np.uint64) + np.uint64(key_offset)
            dists[i, :len(o)] = d[o]
        return (keys, dists, counts), gap
