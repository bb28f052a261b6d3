"""Plain numpy statement of the cross-shard merge (csrc/scan.hip: merge_topk_kernel) for one query, in both orders.
The oracle (oracle/oracle.c: orc_merge_topk) has the ascending form only; tests/test_cpu_exact_edges.py holds this one equal to
it there, so the descending form — the same code with the order of the values reversed — can serve as reference on its own."""
import numpy as np


def f32_orderable(x):
    """uint32 whose unsigned order is the order of the floats (common.cuh: f32_orderable)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def merge_ref(keys, dists, counts, k_out, descending=False):
    """keys, dists: [S, k_in]; counts: [S].  The valid prefixes of the S lists, concatenated and ordered by (dist ascending, key
    ascending) — descending: (score descending, key ascending) — cut at k_out.  -> (keys, dists) of at most k_out entries."""
    keys = np.ascontiguousarray(keys, np.uint64)
    dists = np.ascontiguousarray(dists, np.float32)
    S, k_in = keys.shape
    valid = np.arange(k_in)[None, :] < np.minimum(np.asarray(counts, np.int64), k_in)[:, None]
    ck, cd = keys[valid], dists[valid]
    o = f32_orderable(cd)
    if descending:
        o = ~o
    order = np.lexsort((ck, o))[:k_out]  # last key is the primary one
    return ck[order], cd[order]
