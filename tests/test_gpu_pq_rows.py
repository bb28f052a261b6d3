"""-m gpu: PQ rows (include/leann_backend.h "PQ rows", csrc/scan_pq.hip) against tests/pq_rows_ref.py.  Every comparison is an integer
equality — codes, keys, (float)t bits, counts, the unused tail, codebook bytes — on inputs of small integers, whose distances are exact
and whose ties are real; the refined search equals leann_rerank_batch_device on the same exact rows bit for bit."""
import ctypes as C

import numpy as np
import pytest

import pq_rows_ref as ref
from test_cpu_pq_rows import edge_queries, inputs
from test_gpu_bit_rows import _rerank, _same

pytestmark = pytest.mark.gpu
INVALID, TILE = 1, 2048  # TILE: rows of a score workgroup (csrc/scan_pq.hip: 256 threads x 8 rows)


def _check(la, X, Q, Cb, dsub, fetch_k, what, allow=None, key_offset=0):
    b = la.PqRows.from_host(X, Cb, dsub, key_offset=key_offset)
    codes = b.export()
    assert (codes == la.pq_encode(X, Cb, dsub)).all() and (codes == ref.encode(X, Cb, dsub)).all(), f"{what}: codes differ"
    want = ref.search(codes, Q, Cb, dsub, fetch_k, allow, key_offset)
    _same(b.search_batch(Q, fetch_k, allow), want, what)
    b.close()
    return want


# around the 64-row block of the layout and the 256-row encode tile; one sub-space, M = 9, a ragged last sub-space, 768 x 8
@pytest.mark.parametrize("n, dims, dsub", [(n, 100, 8) for n in (1, 63, 64, 65, 255, 256, 257)] + [(65, 4, 4), (65, 36, 4), (65, 768, 8)])
def test_encode(la, gpu, n, dims, dsub):
    X, _, Cb = inputs(n, 1, dims, dsub)
    X[n // 2, dims // 2] = np.nan  # counts as 0
    want = la.pq_encode(X, Cb, dsub)
    b = la.PqRows.from_host(X, Cb, dsub)
    assert (b.len(), b.dims(), b.dsub(), b.pitch()) == (n, dims, dsub, ref.shape(dims, dsub)[1])
    assert (b.export() == want).all() and (want == ref.encode(X, Cb, dsub)).all()
    assert (b.codebooks() == ref.codebooks(Cb, dims, dsub)).all()
    b.close()
    ld = dims + 5  # garbage, a NaN among it, in the padding columns must not leak into the codes
    P = np.full((n, ld), 7e9, np.float32)
    P[:, :dims], P[::2, dims] = X, np.nan
    dP = la.DeviceArray.from_host(P)
    b = la.PqRows.from_device(dP.ptr, n, dims, ld, Cb, dsub)
    assert (b.export() == want).all()
    b.close()


# M = 1, 9, 13 (a ragged slice), 96 (several slices); rows at the score tile - 1, the tile, the tile + 1, and one row (fetch_k > n);
# 1, 8, 9 and 17 queries around the 8-query table group, plus the four edge queries: one without tables inside every batch
@pytest.mark.parametrize("n, nq, dims, dsub", [(TILE + 1, 9, 8, 8), (TILE - 1, 1, 36, 4), (TILE, 8, 100, 8), (TILE + 1, 17, 768, 8), (1, 9, 100, 8)])
def test_search(la, gpu, n, nq, dims, dsub):
    X, Q, Cb = inputs(n, nq, dims, dsub)
    Q = np.concatenate([Q[:nq // 2], edge_queries(dims, dsub), Q[nq // 2:]])
    k, s, c = _check(la, X, Q, Cb, dsub, 40, f"n={n} nq={nq} dims={dims}", key_offset=2 ** 32 + 7)
    e = nq // 2  # the edge queries: no tables; all-zero tables: every score ties, the first positions win; ..; the unit vectors
    assert c[e] == 0 and (k[e] == ref.NO_KEY).all() and (k[e + 1, :min(n, 40)] == 2 ** 32 + 7 + np.arange(min(n, 40))).all()
    assert k[e + 3, 0] == 2 ** 32 + 7 and s[e + 3, 0] == ref.shape(dims, dsub)[0] * 2 ** 14  # row 0 sits on the centroids whose w is 2^14


def test_score_at_its_maximum(la, gpu):
    X, _, Cb = inputs(130, 1, 4096, 4)  # M = 1024
    X[77] = X[0]
    k, s, c = _check(la, X, edge_queries(4096, 4)[3:], Cb, 4, 130, "maximum")
    assert s[0, 0] == s[0, 1] == 2.0 ** 24 and k[0, :2].tolist() == [0, 77] and s[0, 2] < 2.0 ** 24


# five rows sixty times each: ties go to the lower position; a shared bitmap with stray bits and bytes behind n; no bit set
@pytest.mark.parametrize("share", [None, 0.03, 0.0])
def test_ties_and_bitmaps(la, gpu, share):
    n = 300
    X, Q, Cb = inputs(5, 9, 96, 8)
    X, bm = X[np.arange(n) % 5], None
    if share is not None:
        bm = np.zeros(n // 8 + 9, np.uint8)  # 9 bytes behind ceil(n / 8)
        bits = np.random.default_rng(11).random(n) < share
        bm[:(n + 7) // 8] = np.packbits(bits, bitorder="little")
        bm[(n + 7) // 8 - 1] |= 0xF0  # n % 8 == 4: stray bits behind n in the last byte, and whole stray bytes
        bm[(n + 7) // 8:] = 0xFF
    k, s, c = _check(la, X, Q, Cb, 8, 40, f"share {share}", allow=bm)
    assert (c == (40 if share is None else min(40, bits.sum()))).all()
    if share is None:
        assert (s[0, :39] > s[0, 1:40]).sum() <= 4 and (np.diff(k[0, :40].astype(np.int64)) > 0).all()


def test_emission_path(la, gpu, monkeypatch):
    """70 000 rows, above the select plan's emission threshold (64 Ki): CandEmit; once more on the slab schedule: the same bits"""
    X, Q, Cb = inputs(70000, 8, 32, 4)
    b = la.PqRows.from_host(X, Cb, 4)
    want = ref.search(b.export(), Q, Cb, 4, 40)
    _same(b.search_batch(Q, 40), want, "emit")
    monkeypatch.setenv("LEANN_DEBUG_NO_EMIT", "1")
    la.lib().leann_debug_reload_env()
    _same(b.search_batch(Q, 40), want, "no_emit")
    b.close()


def test_gaussian_rows(la, gpu):
    """real-valued rows and codebooks: the device's code is the float64 argmin wherever the float64 runner-up is further than a
    relative 2 (dsub + 3) 2^-23 — at most 1 % of the sub-vectors may fall outside that (seed 5: none does, checked on the CPU before
    it was committed); the scores are the restatement's on the device's own codes"""
    rng, dsub = np.random.default_rng(5), 8
    X, Q = rng.standard_normal((1500, 768)).astype(np.float32), rng.standard_normal((9, 768)).astype(np.float32)
    Cb = rng.standard_normal((96, 256, 8)).astype(np.float32)
    b = la.PqRows.from_host(X, Cb, dsub)
    codes = b.export()
    S = ref.sub(X, dsub).astype(np.float64)
    clear = 0
    for m in range(96):
        d = ((S[:, m, None, :] - Cb[m][None].astype(np.float64)) ** 2).sum(axis=2)
        two = np.partition(d, 1, axis=1)[:, :2]
        sure = two[:, 1] > two[:, 0] * (1 + 2 * (dsub + 3) * 2.0 ** -23)
        assert (codes[sure, m] == d.argmin(axis=1)[sure]).all()
        clear += sure.sum()
    assert clear >= 0.99 * 1500 * 96
    _same(b.search_batch(Q, 40), ref.search(codes, Q, Cb, dsub, 40), "gaussian rows")
    b.close()


@pytest.mark.parametrize("placement", ["hbm", "host"])
def test_refined(la, gpu, placement):
    n, d, off = 1000, 768, 500
    X, Q, Cb = inputs(n, 17, d, 8)
    b, exact = la.PqRows.from_host(X, Cb, 8, key_offset=off), la.ExactRows.from_host(X, key_offset=off, placement=placement)
    every = np.tile(np.arange(off, off + n, dtype=np.uint64), (len(Q), 1))
    full = _rerank(la, exact, Q, every, np.full(len(Q), n, np.uint32), 10)
    _same(b.search_refined_batch(exact, Q, 10, 1000), full, "fetch_k >= n: the exact top-k")
    cand = ref.search(b.export(), Q, Cb, 8, 40, key_offset=off)
    _same(b.search_refined_batch(exact, Q, 10, 40), _rerank(la, exact, Q, cand[0], cand[2], 10), "fetch_k = 40")
    dQ = la.DeviceArray.from_host(Q)
    ok, od, oc = la.DeviceArray(len(Q) * 10, np.uint64), la.DeviceArray(len(Q) * 10, np.float32), la.DeviceArray(len(Q), np.uint32)
    b.search_refined_batch_device(exact, dQ.ptr, len(Q), 10, 1000, ok.ptr, od.ptr, oc.ptr)
    _same((ok.to_host().reshape(-1, 10), od.to_host().reshape(-1, 10), oc.to_host()), full, "device form")
    b.close()
    exact.close()


@pytest.mark.parametrize("dims, dsub", [(36, 4), (100, 8)])
def test_trainer(la, gpu, dims, dsub):
    rng = np.random.default_rng(dims)
    X = rng.integers(-3, 4, (700, dims)).astype(np.float32)  # not a multiple of 256: floor(c n / 256), a ragged last pass of the update
    for iters in (0, 1):
        assert (la.pq_train(X, dsub, iters) == ref.train(X, dsub, iters)).all(), f"iters = {iters}"
    assert (la.pq_train(X, dsub, 6) == la.pq_train(X, dsub, 6)).all()
    # planted clusters: the float64 quantisation objective under the test's own nearest assignment must not rise from 0 to 1 to 6
    # iterations by more than the assignment's relative error (Lloyd is monotone in exact arithmetic)
    P = (rng.standard_normal((40, dims)) * 4)[rng.integers(0, 40, 3000)] + rng.standard_normal((3000, dims)) * 0.3
    S, obj = ref.sub(P.astype(np.float32), dsub).astype(np.float64), []
    for iters in (0, 1, 6):
        Cb = la.pq_train(P.astype(np.float32), dsub, iters).astype(np.float64)
        obj.append(sum(((S[:, m, None, :] - Cb[m][None]) ** 2).sum(axis=2).min(axis=1).sum() for m in range(len(Cb))))
    print("objective after 0, 1, 6 iterations:", obj)
    assert obj[1] <= obj[0] * (1 + (dsub + 3) * 2.0 ** -23) and obj[2] <= obj[1] * (1 + (dsub + 3) * 2.0 ** -23)


def test_refusals_and_owned_blocks(la, gpu):
    L = la.lib()
    blocks = L.leann_debug_device_blocks()
    X, Q, Cb = inputs(300, 2, 96, 8)
    b = la.PqRows.from_host(X, Cb, 8, key_offset=100)
    fine = la.ExactRows.from_host(X, key_offset=100)
    wrong = {"dims = 64": la.ExactRows.from_host(X[:, :64].copy(), key_offset=100), "cover positions": la.ExactRows.from_host(X, key_offset=101),
             "device 1": la.ExactRows.from_device(0x1000, 300, 96, 96, device=1, key_offset=100)}
    held = L.leann_debug_device_blocks()

    def refused(word, call, *args):
        with pytest.raises(la.LeannError) as e:
            call(*args)
        assert e.value.code == INVALID and word in str(e.value), str(e.value)

    for word, r in wrong.items():
        refused(word, b.search_refined_batch, r, Q, 2, 4)
    refused("exact rows", b.search_refined_batch, None, Q, 2, 4)
    refused("top_k = 0", b.search_refined_batch, fine, Q, 0, 4)
    refused("top_k = 5", b.search_refined_batch, fine, Q, 5, 4)
    refused("fetch_k = 1025", b.search_refined_batch, fine, Q, 5, 1025)
    refused("fetch_k = 0", b.search_batch, Q, 0)
    fake = 0x1000  # never dereferenced: every call below is refused first
    for i, word in ((0, "pq rows"), (1, "queries"), (5, "keys"), (6, "scores"), (7, "counts")):
        args = [b._h, fake, 2, 4, None, fake, fake, fake, None]
        args[i] = None
        assert L.leann_pq_rows_search_batch_device(*args) == INVALID and word in L.leann_last_error().decode()
    refused("d_rows", la.PqRows.from_device, None, 4, 96, 96, Cb)
    refused("ld = 6", la.PqRows.from_device, fake, 4, 96, 6, Cb)
    refused("dims = 4097", la.PqRows.from_device, fake, 4, 4097, 4100, Cb)
    refused("n = ", la.PqRows.from_device, fake, 2 ** 32 - 1, 96, 96, Cb)
    refused("dsub = 5", la.PqRows.from_device, fake, 4, 96, 96, Cb, 5)
    assert L.leann_pq_train_device(None, 300, 96, 96, 8, 1, 0, Cb.ctypes.data_as(C.POINTER(C.c_float))) == INVALID and "d_rows" in L.leann_last_error().decode()
    assert L.leann_debug_device_blocks() == held  # a refused call owns nothing
    empty = la.PqRows.from_host(np.zeros((0, 96), np.float32), Cb, 8)
    k, s, c = empty.search_batch(Q, 4)
    assert (c == 0).all() and (k == ref.NO_KEY).all() and np.isneginf(s).all()
    assert (b.search_refined_batch(fine, Q, 2, 4)[2] == 2).all()  # a search's scratch goes back with the call
    for o in (empty, b, fine, *wrong.values()):
        o.close()
    assert L.leann_debug_device_blocks() == blocks  # after close nothing is owned any more
