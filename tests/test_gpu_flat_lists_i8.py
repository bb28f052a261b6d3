"""-m gpu: int8 rows searched over per-query position lists and per-query bitmaps (include/leann_backend.h "exhaustive search on int8
rows, per query"; csrc/scan_lists_i8.hip: score_lists_i8_kernel).  Every comparison is an equality — keys, f32 distance bits, counts,
the UINT64_MAX / +inf tail, skipped — with the few lines of numpy below on top of tests/flat_i8_ref.py; the sums are exact integers,
so there is no tolerance to choose.  Handles as in tests/test_gpu_flat_i8.py: int8 rows over a ring graph, the device quantising."""
import numpy as np
import pytest

import flat_i8_ref
from refine_ref import NO_KEY, orderable
from test_gpu_flat_i8 import _handle
from util import synth

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = 1, 5
N, OFF = 700, 1000


def _ref(po, ix, Q, top_k, fetch_k, lists, q_list, removed=(), key_offset=0):
    n = len(ix.c)
    dead = np.zeros(n, bool)
    dead[list(removed)] = True
    keys, dists = np.full((len(Q), top_k), NO_KEY, np.uint64), np.full((len(Q), top_k), np.inf, np.float32)
    counts, skipped = np.zeros(len(Q), np.uint32), np.zeros(len(Q), np.uint32)
    for i, l in enumerate(q_list):
        pos = np.asarray(lists[l], np.int64)
        skipped[i] = (pos >= n).sum()
        pos = pos[pos < n]
        pos = pos[~dead[pos]]  # the valid entries, in list order, a position as often as it is listed
        cq, E = flat_i8_ref.query_codes(Q[i], ix.e)
        if E == flat_i8_ref.NONFINITE or not len(pos):
            continue
        s = ix.c32[pos] @ cq.astype(np.int32)
        cand = pos[np.lexsort((pos, -s.astype(np.float32)))[:fetch_k]]
        d = np.array([po.dist_canon(Q[i], ix.Xq[j]) for j in cand], np.float32)
        order = np.lexsort((cand, orderable(d)))[:top_k]
        counts[i] = len(order)
        keys[i, :len(order)], dists[i, :len(order)] = cand[order].astype(np.uint64) + np.uint64(key_offset), d[order]
    return keys, dists, counts, skipped


def _same(got, want, what=""):
    for g, w, name in zip(got, want, ("keys", "dists", "counts", "skipped")):
        g, w = (g.view(np.uint32), w.view(np.uint32)) if g.dtype == np.float32 else (g, w)
        assert (g == w).all(), f"{what}: {name} differ for queries {np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0][:8]}"


# one, two and twelve k-tiles of 128 codes; the plain, plain and block + pair store layouts
@pytest.mark.parametrize("d", [96, 200, 1500])
def test_chunk_edges_sharing_and_entries(la, po, gpu, d):
    rng = np.random.default_rng(d)
    X = synth(po, N, d)
    if d == 96:
        X[N // 2:] = X[:N // 2]  # every row twice: the lower position wins a tie, in the screen and in the answer
    long_list = rng.permutation(N)[:513].astype(np.uint32)  # unsorted; three chunks, the last of one entry
    long_list[[3, 300, 512]] = [N, N + 5, 0xFFFFFFFF]         # beyond the index: skipped and counted, for every query of the tile
    long_list[[10, 400]] = long_list[5]                       # one position three times, across two chunks
    lists = [np.zeros(0, np.uint32)] + [rng.permutation(N)[:m].astype(np.uint32) for m in (1, 255, 256, 257)] + \
            [long_list, rng.permutation(N)[:300].astype(np.uint32), np.array([7, 699, 12, 7, 350], np.uint32),
             np.arange(100, dtype=np.uint32), np.zeros(0, np.uint32)]  # the last two serve no query
    # lists 0-4: one query each; list 5: nine (a full tile and a lone remainder); list 6: eight; list 7: two; scattered over the batch
    q_list = rng.permutation(np.array([0, 1, 2, 3, 4] + [5] * 9 + [6] * 8 + [7] * 2, np.uint32))
    nq = len(q_list)
    Q = synth(po, nq, d, stream=1)
    of5 = np.flatnonzero(q_list == 5)
    Q[of5[0]] = 0            # all-zero codes: every score ties, the lowest listed positions come back
    Q[of5[1], 5] = np.inf    # no codes: count 0
    removed = sorted({int(long_list[20]), int(lists[3][0]), int(lists[6][7]), 12})
    ix, s = flat_i8_ref.Index(X), _handle(la, X, key_offset=OFF)
    s.remove(np.array(removed, np.uint64) + np.uint64(OFF))
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64)
    dQ, dL = la.DeviceArray.from_host(Q), la.DeviceArray.from_host(np.concatenate(lists))
    for top_k, fetch_k in ((10, 40), (10, 300)):  # 40: below the 256 keys a chunk keeps; 300: above, the chunks' candidates are merged
        want = _ref(po, ix, Q, top_k, fetch_k, lists, q_list, removed, OFF)
        _same(s.search_flat_lists_batch(Q, top_k, fetch_k, lists, q_list), want, f"d={d} fetch_k={fetch_k}")
        dk, dd = la.DeviceArray((nq, top_k), np.uint64), la.DeviceArray((nq, top_k), np.float32)
        dc, ds = la.DeviceArray(nq, np.uint32), la.DeviceArray(nq, np.uint32)
        s.search_flat_lists_batch_device(dQ.ptr, nq, top_k, fetch_k, off, dL.ptr, len(lists), q_list, dk.ptr, dd.ptr, dc.ptr, ds.ptr)
        _same((dk.to_host(), dd.to_host(), dc.to_host(), ds.to_host()), want, f"device form, d={d} fetch_k={fetch_k}")
    keys, dists, counts, skipped = want
    assert (skipped[of5] == 3).all() and skipped.sum() == 27 and counts[of5[1]] == 0
    live5 = long_list[(long_list < N) & ~np.isin(long_list, removed)]
    assert (keys[of5[0]] == np.sort(live5)[:10] + OFF).all()
    # top_k above the valid entries: counts and tail
    assert (counts[q_list == 7] == (~np.isin(lists[7], removed)).sum()).all() and counts[q_list == 1][0] <= 1 and counts[q_list == 0][0] == 0
    # fetch_k = 300 >= the 255 live entries of list 3: the exact top-k over Xq of the list, restated without the screen
    i, pos = int(np.flatnonzero(q_list == 3)[0]), np.setdiff1d(lists[3], removed)
    dist = np.array([po.dist_canon(Q[i], ix.Xq[j]) for j in pos], np.float32)
    order = np.lexsort((pos, orderable(dist)))[:10]
    assert (keys[i] == pos[order] + OFF).all() and (dists[i] == dist[order]).all()
    # q_list = None: query i takes list i
    _same(s.search_flat_lists_batch(Q[:len(lists)], 10, 40, lists), _ref(po, ix, Q[:len(lists)], 10, 40, lists, range(len(lists)), removed, OFF),
          "q_list None")
    s.close()


def test_cast_and_accumulator_range(la, po, gpu):
    """4096 columns in +-{125, 126, 127}, row 0 and the queries all-maximal: the codes are the values, s reaches 127^2 * 4096 > 2^24 (the
    cast rounds) and the int32 accumulator its largest magnitude, with both signs"""
    rng, d, n = np.random.default_rng(3), 4096, 300
    base = rng.choice([-1.0, 1.0], d)
    X = np.tile(base, (n, 1)) * rng.choice([125.0, 126.0, 127.0], (n, d), p=[0.02, 0.03, 0.95])
    X[rng.random(X.shape) < 0.01] *= -1
    X[0] = 127 * base
    X, Q = X.astype(np.float32), np.stack([127 * base, -127 * base]).astype(np.float32)
    ix, s = flat_i8_ref.Index(X), _handle(la, X)
    sc = ix.c32 @ Q[0].astype(np.int32)
    assert (ix.c == X).all() and sc[0] == 127 * 127 * 4096 and (sc.astype(np.float32).astype(np.int64) != sc).any()
    lists = [rng.permutation(n).astype(np.uint32)]
    _same(s.search_flat_lists_batch(Q, 10, 20, lists, [0, 0]), _ref(po, ix, Q, 10, 20, lists, [0, 0]), "saturated")
    s.close()


def test_equals_the_flat_search_and_the_bitmap_form(la, po, gpu):
    d, nq = 200, 6
    rng = np.random.default_rng(7)
    X, Q = synth(po, N, d), synth(po, nq, d, stream=1)
    ix, s = flat_i8_ref.Index(X), _handle(la, X, key_offset=OFF)
    removed = [3, 250, 699]
    s.remove(np.array(removed, np.uint64) + np.uint64(OFF))
    allowed = rng.random((nq, N)) < 0.1
    allowed[2] = False       # an all-zero bitmap
    allowed[3, :600] = True  # three chunks
    lists = [np.flatnonzero(row).astype(np.uint32) for row in allowed]  # duplicate-free, in range
    by_lists = s.search_flat_lists_batch(Q, 10, 40, lists)
    _same(by_lists, _ref(po, ix, Q, 10, 40, lists, range(nq), removed, OFF), "lists")
    nbytes = (N + 7) // 8
    bm = np.full((nq, nbytes + 3), 0xFF, np.uint8)  # stray bits behind n: the rest of the last byte and three more bytes
    bm[:, :nbytes] = np.packbits(allowed, axis=-1, bitorder="little")
    bm[:, N // 8] |= (0xFF << (N % 8)) & 0xFF
    for i in range(nq):  # the flat search of each query alone under its list's bitmap: bit for bit
        _same(s.search_flat_batch(Q[i:i + 1], 10, 40, allow=bm[i, :nbytes]), [a[i:i + 1] for a in by_lists[:3]], f"flat, query {i}")
    _same(s.search_flat_filtered_batch(Q, 10, 40, bm), by_lists[:3], "strided bitmaps")
    assert by_lists[2][2] == 0 and (by_lists[3] == 0).all()
    _same(s.search_flat_filtered_batch(Q, 10, 40, bm[3]), s.search_flat_batch(Q, 10, 40, allow=bm[3]), "allow_stride = 0")
    s.close()


def test_refusals(la, po, gpu):
    X, Q = synth(po, N, 96), synth(po, 3, 96, stream=1)
    f32 = _handle(la, X, la.RowType.F32)
    i8, bf16 = f32.to_rows(la.RowType.I8), f32.to_rows(la.RowType.BF16)
    comp = la.ShardedIndex.from_searchers([i8], take_ownership=False).as_backend()
    lists = [np.arange(40, dtype=np.uint32), np.arange(500, 900, dtype=np.uint32), np.array([5], np.uint32)]
    bm = np.zeros((3, (N + 7) // 8), np.uint8)
    for h, words in ((f32, ("f32 rows", "leann_backend_search_filtered_exact_batch")), (bf16, ("bf16 rows", "leann_backend_search_refined_batch")),
                     (comp, ("composite handle", "leann_merge_topk_device"))):
        for call in (lambda: h.search_flat_lists_batch(Q, 2, 4, lists), lambda: h.search_flat_filtered_batch(Q, 2, 4, bm)):
            with pytest.raises(la.LeannError) as e:
                call()
            assert e.value.code == UNSUPPORTED and all(w in str(e.value) for w in words), str(e.value)
    before = i8.search_flat_lists_batch(Q, 10, 40, lists)
    dQ, dL = la.DeviceArray.from_host(Q), la.DeviceArray.from_host(np.concatenate(lists))
    dk, dd, dc = la.DeviceArray((3, 1025), np.uint64), la.DeviceArray((3, 1025), np.float32), la.DeviceArray(3, np.uint32)
    good = [0, 40, 440, 441]
    bad = [("top_k = 0", 0, 40, good, None), ("fetch_k = 1025", 10, 1025, good, None), ("top_k = 41", 41, 40, good, None),
           ("list_off[2]", 10, 40, [0, 440, 40, 441], None), ("list_off[0]", 10, 40, [1, 40, 440, 441], None),
           ("q_list[1]", 10, 40, good, [0, 3, 1]), ("n_lists = 2", 10, 40, [0, 40, 441], None)]
    for word, top_k, fetch_k, off, q_list in bad:
        with pytest.raises(la.LeannError) as e:
            i8.search_flat_lists_batch_device(dQ.ptr, 3, top_k, fetch_k, off, dL.ptr, len(off) - 1, q_list, dk.ptr, dd.ptr, dc.ptr)
        assert e.value.code == INVALID and word in str(e.value), str(e.value)
    dB = la.DeviceArray.from_host(bm)
    with pytest.raises(la.LeannError) as e:  # bitmaps that overlap
        i8.search_flat_filtered_batch_device(dQ.ptr, 3, 10, 40, dB.ptr, bm.shape[1] - 1, dk.ptr, dd.ptr, dc.ptr)
    assert e.value.code == INVALID and "allow_stride" in str(e.value)
    _same(i8.search_flat_lists_batch(Q, 10, 40, lists), before, "the handle answers as before")
    for x in (comp, bf16, i8, f32):
        x.close()
