"""-m gpu: exact top-k over per-query position lists (csrc/scan_lists.hip: score_lists_kernel) — the lists call itself, the
strided-bitmap exact search that is routed through it, and its refusals.

Everything is exact: keys, f32 distance bits, counts and the UINT64_MAX / +inf tail equal po.scan_topk(mode=1) — the k-ordered fmaf
chain — under the bitmap of each list's valid entries, distance = 1 - score."""
import numpy as np
import pytest

from test_gpu_filtered import _exact_oracle
from util import synth

pytestmark = pytest.mark.gpu

U64MAX = np.iinfo(np.uint64).max
INVALID, UNSUPPORTED = 1, 5
GUARD = 64  # NaN floats in front of and behind the row image and the queries: a read outside them is a NaN score
N, OFF, QT = 3001, 1000, 8


def _guarded(la, a):
    flat = np.full(GUARD + a.size + GUARD, np.nan, np.float32)
    flat[GUARD: GUARD + a.size] = a.ravel()
    dev = la.DeviceArray.from_host(flat)
    return dev, dev.ptr + 4 * GUARD


def _handle(la, X, ld, key_offset=OFF):
    img = np.zeros((len(X), ld), np.float32)  # (a handle's pad columns are zero)
    img[:, : X.shape[1]] = X
    keep, ptr = _guarded(la, img)
    return keep, la.BackendSearcher.build_device(la.BackendType.Hnsw, ptr, len(X), X.shape[1], ld, 8, 32, key_offset=key_offset)


def _expected(po, X, Q, k, lists, q_list, key_offset=OFF):
    """per query: the oracle under the bitmap of its list's positions < n, every position repeated as often as it is listed"""
    n = len(X)
    keys, dists = np.full((len(Q), k), U64MAX, np.uint64), np.full((len(Q), k), np.inf, np.float32)
    counts, skipped = np.zeros(len(Q), np.uint32), np.zeros(len(Q), np.uint32)
    for i, l in enumerate(q_list):
        pos = np.asarray(lists[l], np.int64)
        skipped[i] = (pos >= n).sum()
        times = np.bincount(pos[pos < n], minlength=n)
        rk, rs = po.scan_topk(X, Q[i], k, mode=1, allow_mask=np.packbits(times > 0, bitorder="little"))
        rep = times[rk.astype(np.int64)]
        rk, rs = np.repeat(rk, rep)[:k], np.repeat(rs, rep)[:k]
        keys[i, : len(rk)], dists[i, : len(rk)], counts[i] = rk + np.uint64(key_offset), np.float32(1.0) - rs, len(rk)
    return keys, dists, counts, skipped


def _same(got, want):
    for g, w, what in zip(got, want, ("keys", "dists", "counts", "skipped")):
        g, w = (g.view(np.uint32), w.view(np.uint32)) if g.dtype == np.float32 else (g, w)
        assert (g == w).all(), f"{what} differ for queries {np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0][:8]}"


@pytest.mark.parametrize("d,ld", [(50, 52), (96, 96), (768, 768)], ids=["general", "fast", "fast-768"])
def test_lists_call_edges(la, po, gpu, d, ld):
    rng = np.random.default_rng(d)
    X = synth(po, N, d)
    long_list = rng.permutation(N)[:700].astype(np.uint32)                 # unsorted, three chunks
    long_list[[3, 300, 699]] = [N, N + 5, 0xFFFFFFFF]                        # positions beyond the index
    long_list[[10, 520]] = long_list[5]                                      # one position three times, across two chunks
    lists = [np.zeros(0, np.uint32)] + [np.sort(rng.permutation(N)[:m]).astype(np.uint32) for m in (1, 255, 256, 257)] + \
            [long_list, np.array([7, 2999, 3000, 12, 7], np.uint32)]         # the last: shorter than top_k = 10, a duplicate
    # lists 0-4 have one query each, list 5 has QT of them, list 6 QT + 1; the queries of a list are scattered over the batch
    q_list = rng.permutation(np.array([0, 1, 2, 3, 4] + [5] * QT + [6] * (QT + 1), np.uint32))
    nq = len(q_list)
    Q = synth(po, nq, d, stream=1)
    keep_x, s = _handle(la, X, ld)
    keep_q, qptr = _guarded(la, Q)
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64)
    d_lists = la.DeviceArray.from_host(np.concatenate(lists))
    for k in (1, 10, 300):  # 300: more than one chunk's 256 keys
        want = _expected(po, X, Q, k, lists, q_list)
        _same(s.search_exact_lists_batch(Q, k, lists, q_list), want)
        dk, dd = la.DeviceArray((nq, k), np.uint64), la.DeviceArray((nq, k), np.float32)
        dc, ds = la.DeviceArray(nq, np.uint32), la.DeviceArray(nq, np.uint32)
        s.search_exact_lists_batch_device(qptr, nq, k, off, d_lists.ptr, len(lists), q_list, dk.ptr, dd.ptr, dc.ptr, ds.ptr)
        _same((dk.to_host(), dd.to_host(), dc.to_host(), ds.to_host()), want)
    if d == 768:
        # every returned score against the float64 dot: a length-d f32 fma chain is within d * 2^-24 * sum |x_j q_j| of it, and
        # dist = fl(1 - score) adds |dist| * 2^-24 / (1 - 2^-24)
        keys, dists, counts, _ = want
        for i in range(nq):
            rows = X[(keys[i, : counts[i]] - np.uint64(OFF)).astype(np.int64)].astype(np.float64)
            exact = rows @ Q[i].astype(np.float64)
            bound = d * 2.0 ** -24 * (np.abs(rows) * np.abs(Q[i].astype(np.float64))).sum(axis=1)
            dist = dists[i, : counts[i]].astype(np.float64)
            assert (np.abs((1.0 - dist) - exact) <= bound + np.abs(dist) * 2.0 ** -24 / (1 - 2.0 ** -24)).all(), f"query {i}"
    # q_list = None: query i takes list i
    _same(s.search_exact_lists_batch(Q[: len(lists)], 10, lists), _expected(po, X, Q[: len(lists)], 10, lists, range(len(lists))))
    s.close()


def test_strided_bitmaps_take_the_lists_path(la, po, gpu):
    d, nq, k = 96, 6, 10
    rng = np.random.default_rng(7)
    X, Q = synth(po, N, d), synth(po, nq, d, stream=1)
    keep, s = _handle(la, X, d)
    allowed = rng.random((nq, N)) < 0.1
    allowed[2] = False                                      # an all-zero bitmap row
    allowed[3, :600] = True                                 # three chunks
    bm = np.full((nq, (N + 7) // 8 + 3), 0xFF, np.uint8)     # stray bits behind n: the rest of the last byte and three more bytes
    bm[:, : (N + 7) // 8] = np.packbits(allowed, axis=-1, bitorder="little")
    bm[:, N // 8] |= (0xFF << (N % 8)) & 0xFF
    lists = [np.flatnonzero(row).astype(np.uint32) for row in allowed]
    for removed in (None, np.flatnonzero(allowed[3])[:5]):
        if removed is not None:
            assert s.remove(removed.astype(np.uint64) + np.uint64(OFF)) == 5
            allowed[:, removed] = False                     # (for the oracle; the calls below get the lists and bitmaps of before)
        got = s.search_filtered_exact_batch(Q, k, bm)
        by_lists = s.search_exact_lists_batch(Q, k, lists)
        _same(got, by_lists[:3])
        ok, od, oc = _exact_oracle(po, X, Q, k, np.packbits(allowed, axis=-1, bitorder="little"))
        _same(got, (np.where(ok == U64MAX, ok, ok + np.uint64(OFF)), od, oc))
        assert got[2][2] == 0 and (by_lists[3] == 0).all()   # removed positions are skipped, not counted as beyond the index
    s.close()


def test_refusals(la, po, gpu):
    d, k = 96, 10
    X, Q = synth(po, N, d), synth(po, 3, d, stream=1)
    keep, f = _handle(la, X, d)
    lists = [np.arange(40, dtype=np.uint32), np.arange(500, 900, dtype=np.uint32), np.array([5], np.uint32)]
    before = f.search_exact_lists_batch(Q, k, lists)
    bf16, i8 = f.to_rows(la.RowType.BF16), f.to_rows(la.RowType.I8)
    comp = la.ShardedIndex.from_searchers([f], take_ownership=False).as_backend()
    for s, words in ((bf16, "bf16 rows (use the filtered walk"), (i8, "int8 rows (use the filtered walk"), (comp, "composite")):
        with pytest.raises(la.LeannError) as e:
            s.search_exact_lists_batch(Q, k, lists)
        assert e.value.code == UNSUPPORTED and words in str(e.value)
    dQ, dL = la.DeviceArray.from_host(Q), la.DeviceArray.from_host(np.concatenate(lists))
    dk, dd, dc = la.DeviceArray((3, 1025), np.uint64), la.DeviceArray((3, 1025), np.float32), la.DeviceArray(3, np.uint32)
    bad = [("top_k", 1025, [0, 40, 440, 441], None), ("list_off", k, [0, 440, 40, 441], None), ("list_off", k, [1, 40, 440, 441], None),
           ("q_list", k, [0, 40, 440, 441], [0, 3, 1]), ("n_lists", k, [0, 40, 441], None)]
    for word, top_k, off, q_list in bad:
        with pytest.raises(la.LeannError) as e:
            f.search_exact_lists_batch_device(dQ.ptr, 3, top_k, off, dL.ptr, len(off) - 1, q_list, dk.ptr, dd.ptr, dc.ptr)
        assert e.value.code == INVALID and word in str(e.value)
        _same(f.search_exact_lists_batch(Q, k, lists), before)  # the handle answers as before
    for x in (comp, bf16, i8, f):
        x.close()
