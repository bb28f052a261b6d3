"""Numpy restatement of leann_rerank_batch_device (include/leann_backend.h "refining results on exact rows").

Query q has the candidates keys[q, i], i < min(counts[q], fetch_k).  A candidate is valid when key_offset <= key < key_offset + n; the
others are skipped and counted.  The valid ones are scored with po.dist_canon(Q[q], X[key - key_offset]) — the distance the f32
traversal computes — and stable-sorted by (distance bits as ordered f32, key); the first top_k are the answer, the tail of every output
row holds UINT64_MAX / +inf.  A key listed twice is scored and returned twice."""
import numpy as np

NO_KEY = np.iinfo(np.uint64).max


def orderable(d):
    """f32 -> u32 whose unsigned order is the total order the device sorts distances by (csrc/common.cuh f32_orderable)"""
    u = np.asarray(d, np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000).astype(np.uint64)


def rerank(po, X, Q, keys, counts, top_k, key_offset=0):
    """-> (keys [nq x top_k] u64, dists [nq x top_k] f32, counts [nq] u32, skipped [nq] u32)"""
    X = np.ascontiguousarray(X, np.float32)
    Q = np.ascontiguousarray(Q, np.float32)
    keys = np.asarray(keys, np.uint64)
    nq, fetch_k = keys.shape
    n = X.shape[0]
    ok = np.full((nq, top_k), NO_KEY, np.uint64)
    od = np.full((nq, top_k), np.inf, np.float32)
    oc = np.zeros(nq, np.uint32)
    sk = np.zeros(nq, np.uint32)
    for q in range(nq):
        m = min(int(counts[q]), fetch_k)
        cand = [int(k) for k in keys[q, :m]]
        valid = [k for k in cand if key_offset <= k < key_offset + n]
        sk[q] = m - len(valid)
        if not valid:
            continue
        d = np.array([po.dist_canon(Q[q], X[k - key_offset]) for k in valid], np.float32)
        order = np.lexsort((np.array(valid, np.uint64), orderable(d)))[:top_k]  # stable, by (distance, key)
        oc[q] = len(order)
        ok[q, : len(order)] = np.array(valid, np.uint64)[order]
        od[q, : len(order)] = d[order]
    return ok, od, oc, sk
