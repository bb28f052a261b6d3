"""-m gpu: the flat search on bf16 rows (include/leann_backend.h "exhaustive search on bf16 rows", csrc/scan_bf16.hip) against
tests/flat_bf16_ref.py.  The screen's f32 sum has no documented order, so no equality here depends on it: a comparison is either with
the exact answer behind a gap precondition asserted from the reference alone, or on inputs whose screen sums are exact in any order.
The handles are bf16 handles over a trivial ring graph (the flat search reads no graph)."""
import ctypes as C

import numpy as np
import pytest

import flat_bf16_ref
from util import SEED, synth

pytestmark = pytest.mark.gpu
UNSUPPORTED, BQ = 5, 64  # BQ: queries of a score tile (csrc/scan_bf16.hip)


def _handle(la, X, row_type, key_offset=0):
    n, deg = len(X), 8
    adj0 = ((np.arange(n)[:, None] + np.arange(1, deg + 1)[None, :]) % n).astype(np.uint32)
    z = np.zeros(n, np.uint32)
    return la.BackendSearcher.from_arrays(la.BackendType.DiskAnn, X, deg, deg, 0, 0, z.astype(np.uint8), z, adj0, np.zeros((0, deg), np.uint32),
                                          key_offset=key_offset, row_type=row_type)


def _bf16(la, X, key_offset=0):
    return _handle(la, X, la.RowType.BF16, key_offset)


def _same(got, ref, what):
    (gk, gd, gc), (rk, rd, rc) = got, ref
    assert (gc == rc).all(), what
    assert (gk == rk).all(), f"{what}: keys differ in {(gk != rk).any(axis=1).sum()} of {len(gk)} queries"
    assert (gd.view(np.uint32) == rd.view(np.uint32)).all(), what  # the tail too: UINT64_MAX / +inf


def _exact(po, ref, s, Q, top_k, fetch_k, what, **rows):
    r, gap = ref.search(po, Q, top_k, fetch_k, exact=True, **rows)
    print(f"{what}: smallest gap / bound = {gap:.1f}")
    assert gap > 1, f"{what}: the precondition fails (gap / bound = {gap}): change the seed, not the bound"
    _same(s.search_flat_bf16_batch(Q, top_k, fetch_k, allow=rows.get("allow")), r, what)
    return r


@pytest.fixture(scope="module")
def cases(la, po, gpu):
    made = {}

    def get(d, n=300):
        if (d, n) not in made:
            X = synth(po, n, d)
            made[d, n] = (X, flat_bf16_ref.Index(X), _bf16(la, X), synth(po, BQ + 1, d, stream=1))
        return made[d, n]

    yield get
    for c in made.values():
        c[2].close()


# store layouts (ldb 128 plain tail; one block + tail; 768; two blocks; two blocks + tail, T = 6; T = 16) x one and two query tiles
@pytest.mark.parametrize("nq", [1, BQ + 1])
@pytest.mark.parametrize("d", [96, 640, 768, 1024, 1500, 4096])
def test_layouts_and_query_tiles(po, cases, d, nq):
    """keys, distance bits, counts and tail equal the exact top-10 by (dist_canon, position).  Smallest gap between the canonical
    distances at ranks 10 and 41 over the 65 queries, in units of the bound 4 ldb 2^-23 max|q| max|x| (CPU, reference alone):
    d = 96: 1091, 640: 180, 768: 178, 1024: 130, 1500: 82, 4096: 29.  (The bitmap test's 46 allowed rows: 685; the emission test: 576.)"""
    X, ref, s, Q = cases(d)
    _exact(po, ref, s, Q[:nq], 10, 40, f"d={d} nq={nq}")


def _integers(rng, n, d):  # every row twice: the lower position wins a tie, in the screen and in the answer
    X = rng.integers(-4, 5, (n, d)).astype(np.float32)
    X[n // 2:] = X[:n // 2]
    Q = rng.integers(-8, 9, (8, d)).astype(np.float32)
    Q[1] = 0                        # every score ties: the candidates are the first fetch_k positions
    Q[2, 5] = np.nan                # no pieces: count 0
    Q[3] *= np.float32(2.0 ** -70)  # exact scaling
    return X, Q


def _lo_piece(rng, n, d):
    """hi = 1 and lo = +-2^-10 for every query element; every row a permutation of one multiset of integers, so sum_j x_ij is the same
    for all rows and only the 2^-10 term orders them.  All sums are multiples of 2^-10 below 2^9: exact in f32 in any order."""
    X = np.stack([rng.permutation(np.arange(d) % 9 - 4) for _ in range(n)]).astype(np.float32)
    Q = (1 + rng.choice([-1.0, 1.0], (8, d)) * 2.0 ** -10).astype(np.float32)
    return X, Q


@pytest.mark.parametrize("make", [_integers, _lo_piece])
def test_order_free_equalities(la, po, make):
    X, Q = make(np.random.default_rng(7), 300, 96)
    ref, s = flat_bf16_ref.Index(X), _bf16(la, X, key_offset=1000)
    assert (ref.Xr == X).all()
    for top_k, fetch_k in ((10, 40), (10, 10), (300, 300), (7, 1024)):
        rk, rd, rc = r = ref.search(po, Q, top_k, fetch_k, key_offset=1000)[0]
        _same(s.search_flat_bf16_batch(Q, top_k, fetch_k), r, (make.__name__, top_k, fetch_k))
        if make is _integers:
            rank = np.argsort(rk[0])  # top_k = 300: where each position stands in the answer; a row comes before its copy
            assert rc[2] == 0 and (rk[1] == 1000 + np.arange(top_k)).all() and (top_k < 300 or (rank[:150] < rank[150:]).all())
        else:  # the reference itself: a screen without lo ties everywhere and would keep the first fetch_k positions
            hi, lo = flat_bf16_ref.split(Q[0])
            assert (hi == 0x3F80).all() and (np.abs(flat_bf16_ref.widen(lo)) == 2.0 ** -10).all()
            assert fetch_k >= 300 or not (np.sort(rk, axis=1)[:, :top_k] == 1000 + np.arange(top_k)).all()
    s.close()


@pytest.mark.parametrize("name", ["3 percent, stray bits", "fewer than top_k", "none", "bitmap and removals"])
def test_bitmap_and_removals(la, po, cases, name):
    X, ref, s, Q = cases(768, 1500)
    n, removed = 1500, ()
    bm = np.zeros(n // 8 + 9, np.uint8)  # 9 bytes behind ceil(n / 8)
    bits = np.random.default_rng(11).random(n) < {"fewer than top_k": 0.004, "none": 0.0}.get(name, 0.03)
    bm[:(n + 7) // 8] = np.packbits(bits, bitorder="little")
    bm[(n + 7) // 8 - 1] |= 0xF0  # n % 8 == 4: stray bits behind n in the last byte, and whole stray bytes
    bm[(n + 7) // 8:] = 0xFF
    if "removals" in name:  # a handle of its own: removing changes it
        s = _bf16(la, X)
        removed = [int(i) for i in np.flatnonzero(bits)[::3]] + [0, 1499]
        s.remove(np.array(sorted(set(removed)), np.uint64))
    r = _exact(po, ref, s, Q[:9], 10, 40, name, allow=bm, removed=removed)
    assert (r[2] == {"fewer than top_k": bits.sum(), "none": 0}.get(name, 10)).all() and r[2].max() <= 10
    if "removals" in name:
        s.close()


def test_emission_path(la, po, monkeypatch):
    """70 000 rows, above the select plan's emission threshold (64 Ki): CandEmit; once more on the slab schedule: the same bits"""
    X, Q = synth(po, 70000, 128), synth(po, 8, 128, stream=1)
    ref, s = flat_bf16_ref.Index(X), _bf16(la, X)
    r = _exact(po, ref, s, Q, 10, 40, "emit")
    monkeypatch.setenv("LEANN_DEBUG_NO_EMIT", "1")
    la.lib().leann_debug_reload_env()
    _same(s.search_flat_bf16_batch(Q, 10, 40), r, "no_emit")
    s.close()


def test_distance_is_the_walks(cases):  # whatever key the bf16 walk returns on the same handle: the same distance bits
    X, ref, s, Q = cases(768)
    fk, fd, fc = s.search_flat_bf16_batch(Q, 300, 300)
    wk, wd, wc = s.search_batch(Q, 64, 128)
    assert (fc == 300).all() and (wc == 64).all()
    for i in range(len(Q)):
        flat = dict(zip(fk[i].tolist(), fd[i].view(np.uint32).tolist()))
        assert [flat[k] for k in wk[i].tolist()] == wd[i].view(np.uint32).tolist()


def test_refusals_name_the_way_out(la, po, cases):
    X, L = cases(96)[0], la.lib()
    f32 = _handle(la, X, la.RowType.F32)
    dF, dW = la.DeviceArray.from_host(po.synth_features(SEED, 64, 64, 1.0, 0, 0, 600)), la.DeviceArray.from_host(po.synth_weights(SEED, 64, 64))
    r, hb = C.c_void_p(), C.c_void_p()
    la._native.check(L.leann_recompute_create(dF.ptr, 600, 64, dW.ptr, 64, 0, 0, C.byref(r)))
    la._native.check(L.leann_recompute_build_index(r, 0, 8, 64, C.byref(hb)))
    comp = la.ShardedIndex.from_searchers([_bf16(la, X), _bf16(la, X, key_offset=300)], take_ownership=True).as_backend()
    for h, words in ((_handle(la, X, la.RowType.I8), ("int8 rows", "leann_backend_search_flat_batch")), (comp, ("composite handle", "leann_merge_topk_device")),
                     (la.BackendSearcher(hb, la.BackendType.Hnsw), ("recomputes its vectors", "leann_recompute_search_batch_device")),
                     (f32, ("f32 rows", "leann_backend_search_filtered_exact_batch"))):
        blocks = L.leann_debug_device_blocks()
        with pytest.raises(la.LeannError) as e:
            h.search_flat_bf16_batch(np.zeros((2, h.dims()), np.float32), 2, 4)
        assert e.value.code == UNSUPPORTED and all(w in str(e.value) for w in words), str(e.value)
        assert L.leann_debug_device_blocks() == blocks  # a refused call owns nothing
        h.close()
    L.leann_recompute_close(r)
