"""-m gpu: MXFP4 rows (include/leann_backend.h "MXFP4 rows", csrc/scan_mx4.hip) against tests/mx4_rows_ref.py: equality in keys, score
bits, counts and tail on inputs whose sums are exact in any order; on synthetic rows, the summation order being open, consistency
within B = K_pad 2^-22 sum_j |term_j| per (query, row): K_pad f32 additions at unit round-off 2^-23, doubled for the multi-term adder."""
import ctypes as C

import numpy as np
import pytest

import mx4_rows_ref as ref
from test_cpu_mx4_rows import DIMS, rows
from test_gpu_bit_rows import _rerank, _same
from util import synth

pytestmark = pytest.mark.gpu
INVALID, BQ = 1, 64  # BQ: queries of a score tile (csrc/scan_mx4.hip)
G = 2.0 ** -2        # the granularity of a term of exact_inputs: (0.5 * 2^-1) * (1 * 2^0)


def exact_inputs(n, nq, dims, seed=0):
    """rows in {0, +-0.5 .. +-6} 2^c, c in {-1, 0, 1} per block, a 4 or 6 leading every block (scale 2^c, codes exact); queries integers in
    [-14, 14] 2^c', c' in {0, 1}, an 8 .. 14 leading every block (codes exact, 14 * 32 = 448).  sum_j |term_j| <= 4096 * 12 * 28 < 2^24 G."""
    rng, nb = np.random.default_rng(seed + dims), -(-dims // 32)

    def draw(m, values, lead, exps):
        v = rng.choice(values, (m, nb, 32)) * rng.choice([-1.0, 1.0], (m, nb, 32))
        v[:, :, 0] = rng.choice(lead, (m, nb)) * rng.choice([-1.0, 1.0], (m, nb))
        return (v * 2.0 ** rng.choice(exps, (m, nb, 1))).reshape(m, -1)[:, :dims].astype(np.float32)

    return draw(n, ref.E2M1, [4, 6], [-1, 0, 1]), draw(nq, np.arange(15), np.arange(8, 15), [0, 1])


def _reference(X, Q):
    T, A, finite = ref.terms(*ref.pack(X), Q)
    return T, A, finite, 256 * ref.ktiles(X.shape[1])


def _check_exact(la, X, Q, fetch_k, what, allow=None, key_offset=0):
    T, A, finite, _ = _reference(X, Q)
    ref.assert_order_free(A, G)
    b = la.Mx4Rows.from_host(X, key_offset=key_offset)
    want = ref.search(T, finite, fetch_k, allow, key_offset)
    _same(b.search_batch(Q, fetch_k, allow), want, what)
    b.close()
    return want


def _check_within_bound(got, X, Q, fetch_k, what, allow=None):
    """a returned row i displaced a true top row m only if t_i + B_i >= t_m - B_m; a row r is missing only if a returned j has t_j + B_j >= t_r - B_r"""
    T, A, finite, k_pad = _reference(X, Q)
    B, pos, worst = k_pad * 2.0 ** -22 * A, ref.allowed(len(X), allow), 0.0
    keys, scores, counts = got
    for q in range(len(Q)):
        m = min(fetch_k, len(pos)) if finite[q] else 0
        assert counts[q] == m and (keys[q, m:] == ref.NO_KEY).all() and np.isneginf(scores[q, m:]).all(), what
        if m == 0:
            continue
        at, s, t = keys[q, :m].astype(np.int64), scores[q, :m].astype(np.float64), T[q]
        assert len(set(at)) == m and np.isin(at, pos).all() and (np.diff(s) <= 0).all(), what
        worst = max(worst, (np.abs(s - t[at]) / np.maximum(B[q, at], 1e-300)).max())
        assert (np.abs(s - t[at]) <= B[q, at]).all(), f"{what}: a score is {worst} B off its reference"
        top = pos[np.argsort(-t[pos], kind="stable")[:m]]
        missing = np.setdiff1d(pos, at)
        assert (t[at] >= t[top[-1]] - B[q, at] - B[q, top].max()).all(), what
        assert (t[missing] <= t[top[-1]] + B[q, missing] + B[q, at].max()).all(), what
    print(f"{what}: largest |score - reference| = {worst:.3g} B")


@pytest.mark.parametrize("dims", DIMS)
def test_pack(la, gpu, dims):
    X = rows(dims)  # 37 rows: not a multiple of the pack kernel's 4 rows per workgroup
    want = la.pack_mx4(X)
    b = la.Mx4Rows.from_host(X)
    assert (b.len(), b.dims()) == (37, dims) and all((g == w).all() for g, w in zip(b.export(), want))
    b.close()
    ld = dims + 5  # garbage, a NaN among it, in the padding columns must not leak into codes or scales
    P = np.full((37, ld), 7e9, np.float32)
    P[:, :dims], P[::2, dims] = X, np.nan
    dP = la.DeviceArray.from_host(P)
    b = la.Mx4Rows.from_device(dP.ptr, 37, dims, ld)
    assert all((g == w).all() for g, w in zip(b.export(), want))
    b.close()


# one block, a ragged block, one k-tile, a ragged k-tile, whole k-tiles up to the widest row x one and two query tiles; row-tile edges
@pytest.mark.parametrize("n, nq, dims", [(257, nq, d) for d in (32, 100, 256, 288, 768, 1024, 4096) for nq in (1, BQ + 1)]
                         + [(n, 3, 288) for n in (1, 127, 128, 129, 257)])
def test_order_free(la, gpu, n, nq, dims):
    _check_exact(la, *exact_inputs(n, nq, dims), 40, f"n={n} nq={nq} dims={dims}")


@pytest.mark.parametrize("fetch_k", [1, 40, 1024])
def test_ties_and_limits(la, gpu, fetch_k):
    X, Q = exact_inputs(5, 4, 96)
    X = X[np.arange(300) % 5]  # five rows, sixty times each: ties go to the lower position
    Q[1] = 0                   # all-zero codes: every score ties, the candidates are the first positions
    Q[2, 5] = np.nan           # no codes: count 0
    k, s, c = _check_exact(la, X, Q, fetch_k, fetch_k, key_offset=2 ** 32 + 7)
    m = min(fetch_k, 300)  # 1 024 is above n
    assert c.tolist() == [m, m, 0, m] and (k[1, :m] == 2 ** 32 + 7 + np.arange(m)).all() and (k[2] == ref.NO_KEY).all()
    assert (s[0, :m - 1] > s[0, 1:m]).sum() <= 4 and (np.diff(k[0, :min(m, 60)].astype(np.int64)) > 0).all()


# no bitmap; then 3 percent allowed with stray bits and bytes behind n, fewer than fetch_k, none, all
@pytest.mark.parametrize("n, dims, share", [(1500, 768, None), (300, 4096, None), (1500, 768, 0.03), (1500, 768, 0.01), (1500, 768, 0.0), (1500, 768, 1.0)])
def test_synthetic_rows_and_bitmaps(la, po, gpu, n, dims, share):
    X, Q, bm, bits = synth(po, n, dims), synth(po, 9, dims, stream=1), None, np.ones(n, bool)
    if share is not None:
        bm = np.zeros(n // 8 + 9, np.uint8)  # 9 bytes behind ceil(n / 8)
        bits = np.random.default_rng(11).random(n) < share
        bm[:(n + 7) // 8] = np.packbits(bits, bitorder="little")
        bm[(n + 7) // 8 - 1] |= 0xF0  # n % 8 == 4: stray bits behind n in the last byte, and whole stray bytes
        bm[(n + 7) // 8:] = 0xFF
    b = la.Mx4Rows.from_host(X)
    got = b.search_batch(Q, 40, bm)
    _check_within_bound(got, X, Q, 40, f"{n} x {dims}, share {share}", allow=bm)
    assert (got[2] == min(40, bits.sum())).all()
    b.close()


def test_emission_path(la, po, gpu, monkeypatch):
    """70 000 rows, above the select plan's emission threshold (64 Ki): CandEmit; once more on the slab schedule: the same bits"""
    X, Q = synth(po, 70000, 256), synth(po, 8, 256, stream=1)
    b = la.Mx4Rows.from_host(X)
    emit = b.search_batch(Q, 40)
    _check_within_bound(emit, X, Q, 40, "emit")
    monkeypatch.setenv("LEANN_DEBUG_NO_EMIT", "1")
    la.lib().leann_debug_reload_env()
    _same(b.search_batch(Q, 40), emit, "no_emit against emit")
    b.close()


@pytest.mark.parametrize("placement", ["hbm", "host"])
def test_refined(la, gpu, placement):
    n, d, off = 1000, 768, 500
    X, Q = exact_inputs(n, BQ + 1, d)
    b, exact = la.Mx4Rows.from_host(X, key_offset=off), la.ExactRows.from_host(X, key_offset=off, placement=placement)
    every = np.tile(np.arange(off, off + n, dtype=np.uint64), (len(Q), 1))
    full = _rerank(la, exact, Q, every, np.full(len(Q), n, np.uint32), 10)
    _same(b.search_refined_batch(exact, Q, 10, 1000), full, "fetch_k >= n: the exact top-k")
    T, A, finite, _ = _reference(X, Q)
    ref.assert_order_free(A, G)
    cand = ref.search(T, finite, 40, key_offset=off)
    _same(b.search_refined_batch(exact, Q, 10, 40), _rerank(la, exact, Q, cand[0], cand[2], 10), "fetch_k = 40")
    dQ = la.DeviceArray.from_host(Q)
    ok, od, oc = la.DeviceArray(len(Q) * 10, np.uint64), la.DeviceArray(len(Q) * 10, np.float32), la.DeviceArray(len(Q), np.uint32)
    b.search_refined_batch_device(exact, dQ.ptr, len(Q), 10, 1000, ok.ptr, od.ptr, oc.ptr)
    _same((ok.to_host().reshape(-1, 10), od.to_host().reshape(-1, 10), oc.to_host()), full, "device form")
    b.close()
    exact.close()


def test_refusals(la, po, gpu):
    L, X, Q = la.lib(), synth(po, 300, 96), synth(po, 2, 96, stream=1)
    b = la.Mx4Rows.from_host(X, key_offset=100)
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
    for i, word in ((0, "mx4 rows"), (1, "queries"), (5, "keys"), (6, "scores"), (7, "counts")):
        args = [b._h, fake, 2, 4, None, fake, fake, fake, None]
        args[i] = None
        assert L.leann_mx4_rows_search_batch_device(*args) == INVALID and word in L.leann_last_error().decode()
    out = C.c_void_p()
    assert L.leann_mx4_rows_from_device(None, 4, 8, 8, 0, 0, C.byref(out)) == INVALID and "d_rows" in L.leann_last_error().decode()
    assert L.leann_mx4_rows_from_device(fake, 4, 8, 6, 0, 0, C.byref(out)) == INVALID and "ld = 6" in L.leann_last_error().decode()
    assert L.leann_mx4_rows_from_device(fake, 4, 4097, 4100, 0, 0, C.byref(out)) == INVALID and "dims = 4097" in L.leann_last_error().decode()
    assert L.leann_mx4_rows_from_device(fake, 2 ** 32 - 1, 8, 8, 0, 0, C.byref(out)) == INVALID and "n = " in L.leann_last_error().decode()
    assert L.leann_debug_device_blocks() == blocks  # a refused call owns nothing
    empty = la.Mx4Rows.from_host(np.zeros((0, 96), np.float32))
    k, s, c = empty.search_batch(Q, 4)
    assert (c == 0).all() and (k == ref.NO_KEY).all() and np.isneginf(s).all()
    ring = ((np.arange(300)[:, None] + np.arange(1, 9)) % 300).astype(np.uint32)  # a trivial graph: only the rows matter here
    i8, f32 = (la.BackendSearcher.from_arrays(la.BackendType.DiskAnn, X, 8, 8, 0, 0, np.zeros(300, np.uint8), np.zeros(300, np.uint32), ring,
                                              np.zeros((0, 8), np.uint32), row_type=t) for t in (la.RowType.I8, la.RowType.F32))
    refused("no f32 rows", la.Mx4Rows.from_searcher, i8)
    bs = la.Mx4Rows.from_searcher(f32)
    assert all((g == w).all() for g, w in zip(bs.export(), la.pack_mx4(X)))
    for o in (bs, f32, i8, empty, b, fine, *wrong.values()):
        o.close()
