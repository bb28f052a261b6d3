"""-m gpu: sign-bit rows (include/leann_backend.h "sign-bit rows", csrc/scan_bits.hip).  Every search comparison is an integer equality
with tests/bit_rows_ref.py — keys, score bits, counts, the unused tail — and the refined search equals leann_rerank_batch_device on
the same exact rows bit for bit."""
import ctypes as C

import numpy as np
import pytest

import bit_rows_ref as ref
from test_cpu_bit_rows import rows
from util import synth

pytestmark = pytest.mark.gpu
INVALID, BQ = 1, 64  # BQ: queries of a score tile (csrc/scan_bits.hip)


def _same(got, want, what):
    for g, w, name in zip(got, want, ("keys", "scores", "counts")):
        assert (g.view(np.uint32) == w.view(np.uint32)).all(), f"{what}: {name} differ"


def _check(la, X, Q, fetch_k, what, center=None, allow=None, key_offset=0):
    b = la.BitRows.from_host(X, center, key_offset=key_offset)
    want = ref.search(la, ref.pack(X, center), X.shape[1], Q, fetch_k, allow, key_offset)
    _same(b.search_batch(Q, fetch_k, allow), want, what)
    b.close()
    return want


@pytest.mark.parametrize("dims", [1, 7, 8, 9, 127, 128, 129, 768, 4096])
def test_pack(la, gpu, dims):
    X, c = rows(dims)  # 37 rows: not a multiple of the pack kernel's 4 rows per workgroup
    for center in (None, c):
        b = la.BitRows.from_host(X, center)
        assert (b.len(), b.dims(), b.pitch()) == (37, dims, ref.pitch(dims)) and (b.export() == la.pack_sign_bits(X, center)).all()
        b.close()
    ld = dims + 5  # garbage, a NaN among it, in the padding columns must not leak into bits
    P = np.full((37, ld), 7.0, np.float32)
    P[:, :dims], P[::2, dims] = X, np.nan
    dP, dc = la.DeviceArray.from_host(P), la.DeviceArray.from_host(c)
    b = la.BitRows.from_device(dP.ptr, 37, dims, ld, dc.ptr)
    assert (b.export() == la.pack_sign_bits(X, c)).all()
    b.close()


# one k-tile, a ragged tail inside a k-tile, whole tiles, and both sides of the 2 048 columns resident in LDS x one and two query tiles
@pytest.mark.parametrize("nq", [1, BQ + 1])
@pytest.mark.parametrize("dims", [1, 100, 128, 136, 768, 1024, 4096])
def test_layouts_and_query_tiles(la, po, gpu, dims, nq):
    _check(la, synth(po, 1500, dims), synth(po, nq, dims, stream=1), 40, f"dims={dims} nq={nq}")


@pytest.mark.parametrize("n", [1, 127, 128, 129, 257])
def test_row_tile_edges(la, po, gpu, n):
    _check(la, synth(po, n, 128), synth(po, 3, 128, stream=1), 40, f"n={n}", center=synth(po, 1, 128, stream=2)[0] * 0.1)


@pytest.mark.parametrize("fetch_k", [1, 40, 1024])
def test_ties_and_limits(la, po, gpu, fetch_k):
    X = synth(po, 5, 96)[np.arange(300) % 5]  # five patterns, sixty times each: ties go to the lower position
    Q = synth(po, 4, 96, stream=1)
    Q[1] = 0          # all-zero codes: every score ties, the candidates are the first positions
    Q[2, 5] = np.nan  # no codes: count 0
    k, s, c = _check(la, X, Q, fetch_k, fetch_k, key_offset=2 ** 32 + 7)
    m = min(fetch_k, 300)  # 1 024 is above n
    assert c.tolist() == [m, m, 0, m] and (k[1, :m] == 2 ** 32 + 7 + np.arange(m)).all() and (k[2] == ref.NO_KEY).all()
    assert (s[0, :m - 1] > s[0, 1:m]).sum() <= 4 and (np.diff(k[0, :min(m, 60)].astype(np.int64)) > 0).all()


def test_score_at_its_maximum(la, gpu):
    X, Q = np.ones((130, 4096), np.float32), np.full((1, 4096), -127, np.float32)  # amax = 127: E = 0, every code is -127
    X[7, 1000:] = -1  # one row below the maximum
    k, s, c = _check(la, X, Q, 130, "maximum")
    assert s[0, 0] == -127 * 1000 and k[0, 0] == 7 and (s[0, 1:] == -127 * 4096).all()


@pytest.mark.parametrize("name, share", [("3 percent, stray bits", 0.03), ("fewer than fetch_k", 0.01), ("none", 0.0), ("all", 1.0)])
def test_bitmaps(la, po, gpu, name, share):
    n = 1500
    bm = np.zeros(n // 8 + 9, np.uint8)  # 9 bytes behind ceil(n / 8)
    bits = np.random.default_rng(11).random(n) < share
    bm[:(n + 7) // 8] = np.packbits(bits, bitorder="little")
    bm[(n + 7) // 8 - 1] |= 0xF0  # n % 8 == 4: stray bits behind n in the last byte, and whole stray bytes
    bm[(n + 7) // 8:] = 0xFF
    k, s, c = _check(la, synth(po, n, 768), synth(po, 9, 768, stream=1), 40, name, allow=bm)
    assert (c == min(40, bits.sum())).all()


def test_emission_path(la, po, gpu, monkeypatch):
    """70 000 rows, above the select plan's emission threshold (64 Ki): CandEmit; once more on the slab schedule: the same bits"""
    X, Q = synth(po, 70000, 128), synth(po, 8, 128, stream=1)
    b, want = la.BitRows.from_host(X), ref.search(la, ref.pack(X), 128, Q, 40)
    _same(b.search_batch(Q, 40), want, "emit")
    monkeypatch.setenv("LEANN_DEBUG_NO_EMIT", "1")
    la.lib().leann_debug_reload_env()
    _same(b.search_batch(Q, 40), want, "no_emit")
    b.close()


def _rerank(la, rows_, Q, keys, counts, top_k):
    fetch_k = keys.shape[1]
    dQ, dK, dC = la.DeviceArray.from_host(Q), la.DeviceArray.from_host(keys), la.DeviceArray.from_host(counts)
    ok, od, oc = la.DeviceArray(len(Q) * top_k, np.uint64), la.DeviceArray(len(Q) * top_k, np.float32), la.DeviceArray(len(Q), np.uint32)
    la.rerank_batch_device(rows_, dQ.ptr, len(Q), dK.ptr, dC.ptr, fetch_k, top_k, ok.ptr, od.ptr, oc.ptr)
    la.sync()
    return ok.to_host().reshape(len(Q), top_k), od.to_host().reshape(len(Q), top_k), oc.to_host()


@pytest.mark.parametrize("placement", ["hbm", "host"])
def test_refined(la, po, gpu, placement):
    n, d, off = 1000, 768, 500
    X, Q = synth(po, n, d), synth(po, BQ + 1, d, stream=1)
    c = X.mean(axis=0)
    b, exact = la.BitRows.from_host(X, c, key_offset=off), la.ExactRows.from_host(X, key_offset=off, placement=placement)
    every = np.tile(np.arange(off, off + n, dtype=np.uint64), (len(Q), 1))
    full = _rerank(la, exact, Q, every, np.full(len(Q), n, np.uint32), 10)
    _same(b.search_refined_batch(exact, Q, 10, 1000), full, "fetch_k >= n: the exact top-k")
    cand = ref.search(la, ref.pack(X, c), d, Q, 40, key_offset=off)
    _same(b.search_refined_batch(exact, Q, 10, 40), _rerank(la, exact, Q, cand[0], cand[2], 10), "fetch_k = 40")
    dQ = la.DeviceArray.from_host(Q)
    ok, od, oc = la.DeviceArray(len(Q) * 10, np.uint64), la.DeviceArray(len(Q) * 10, np.float32), la.DeviceArray(len(Q), np.uint32)
    b.search_refined_batch_device(exact, dQ.ptr, len(Q), 10, 1000, ok.ptr, od.ptr, oc.ptr)
    _same((ok.to_host().reshape(-1, 10), od.to_host().reshape(-1, 10), oc.to_host()), full, "device form")
    b.close()
    exact.close()


def test_refusals(la, po, gpu):
    L, X, Q = la.lib(), synth(po, 300, 96), synth(po, 2, 96, stream=1)
    b = la.BitRows.from_host(X, key_offset=100)
    fine = la.ExactRows.from_host(X, key_offset=100)
    wrong = {"dims = 64": la.ExactRows.from_host(X[:, :64].copy(), key_offset=100), "cover positions": la.ExactRows.from_host(X, key_offset=101),
             "device 1": la.ExactRows.from_device(0x1000, 300, 96, 96, device=1, key_offset=100)}
    blocks = L.leann_debug_device_blocks()

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
    for i, word in ((0, "bit rows"), (1, "queries"), (5, "keys"), (6, "scores"), (7, "counts")):
        args = [b._h, fake, 2, 4, None, fake, fake, fake, None]
        args[i] = None
        assert L.leann_bit_rows_search_batch_device(*args) == INVALID and word in L.leann_last_error().decode()
    out = C.c_void_p()
    assert L.leann_bit_rows_from_device(None, 4, 8, 8, None, 0, 0, C.byref(out)) == INVALID and "d_rows" in L.leann_last_error().decode()
    assert L.leann_bit_rows_from_device(fake, 4, 8, 6, None, 0, 0, C.byref(out)) == INVALID and "ld = 6" in L.leann_last_error().decode()
    assert L.leann_bit_rows_from_device(fake, 4, 4097, 4100, None, 0, 0, C.byref(out)) == INVALID and "dims = 4097" in L.leann_last_error().decode()
    assert L.leann_bit_rows_from_device(fake, 2 ** 32 - 1, 8, 8, None, 0, 0, C.byref(out)) == INVALID and "n = " in L.leann_last_error().decode()
    assert L.leann_debug_device_blocks() == blocks  # a refused call owns nothing
    empty = la.BitRows.from_host(np.zeros((0, 96), np.float32))
    k, s, c = empty.search_batch(Q, 4)
    assert (c == 0).all() and (k == ref.NO_KEY).all() and np.isneginf(s).all()
    ring = ((np.arange(300)[:, None] + np.arange(1, 9)) % 300).astype(np.uint32)  # a trivial graph: only the rows matter here
    i8, f32 = (la.BackendSearcher.from_arrays(la.BackendType.DiskAnn, X, 8, 8, 0, 0, np.zeros(300, np.uint8), np.zeros(300, np.uint32), ring,
                                              np.zeros((0, 8), np.uint32), row_type=t) for t in (la.RowType.I8, la.RowType.F32))
    refused("no f32 rows", la.BitRows.from_searcher, i8)
    bs = la.BitRows.from_searcher(f32)
    assert (bs.export() == la.pack_sign_bits(X)).all()
    for o in (bs, f32, i8, empty, b, fine, *wrong.values()):
        o.close()
