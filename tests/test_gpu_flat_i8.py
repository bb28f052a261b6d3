"""-m gpu: the flat search on int8 rows (include/leann_backend.h "exhaustive search on int8 rows", csrc/scan_i8.hip).  Every comparison
is an equality with tests/flat_i8_ref.py: keys, f32 distance bits, counts and the unused tail.  The handles are int8 handles over a
trivial ring graph (the flat search reads no graph); the device quantises the rows itself."""
import ctypes as C

import numpy as np
import pytest

import flat_i8_ref
from util import SEED, recall_at_k, synth

pytestmark = pytest.mark.gpu
UNSUPPORTED, BQ = 5, 64  # BQ: queries of a score tile (csrc/scan_i8.hip)


def _handle(la, X, row_type=None, key_offset=0):
    n, deg = len(X), 8
    adj0 = ((np.arange(n)[:, None] + np.arange(1, deg + 1)[None, :]) % n).astype(np.uint32)
    z = np.zeros(n, np.uint32)
    return la.BackendSearcher.from_arrays(la.BackendType.DiskAnn, X, deg, deg, 0, 0, z.astype(np.uint8), z, adj0, np.zeros((0, deg), np.uint32),
                                          key_offset=key_offset, row_type=la.RowType.I8 if row_type is None else row_type)


def _same(got, ref, what):
    (gk, gd, gc), (rk, rd, rc) = got, ref
    assert (gc == rc).all(), what
    assert (gk == rk).all(), f"{what}: keys differ in {(gk != rk).any(axis=1).sum()} of {len(gk)} queries"
    assert (gd.view(np.uint32) == rd.view(np.uint32)).all(), what  # the tail too: UINT64_MAX / +inf


@pytest.fixture(scope="module")
def cases(la, po, gpu):
    made = {}

    def get(d, n=300, scaled=False):
        if (d, n, scaled) not in made:
            X = synth(po, n, d)
            if scaled:  # a few columns an order of magnitude above the rest, as the int8 tests build them
                X[:, [3, 100, 400, 700]] *= 12
                X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
            made[d, n, scaled] = (X, flat_i8_ref.Index(X), _handle(la, X), synth(po, BQ + 1, d, stream=1))
        return made[d, n, scaled]

    yield get
    for c in made.values():
        c[2].close()


# store layouts (ldb 128 plain tail; 512-pair + tail; 768; one whole block; block + pair, T = 6; T = 16) x one and two query tiles
@pytest.mark.parametrize("nq", [1, BQ + 1])
@pytest.mark.parametrize("d", [96, 640, 768, 1024, 1500, 4096])
def test_layouts_and_query_tiles(po, cases, d, nq):
    X, ref, s, Q = cases(d)
    _same(s.search_flat_batch(Q[:nq], 10, 40), ref.search(po, Q[:nq], 10, 40), f"d={d} nq={nq}")


def test_ties_degenerate_queries_and_fetch_limits(la, po, cases):
    X = synth(po, 300, 96)
    X[150:] = X[:150]  # every row twice: the lower position wins a tie, in the screen and in the answer
    ref, s, Q = flat_i8_ref.Index(X), _handle(la, X, key_offset=1000), synth(po, 8, 96, stream=1)
    Q[1] = 0       # all-zero codes: every score ties, the candidates are the first fetch_k positions
    Q[2, 5] = np.nan  # no codes: count 0
    Q[3] *= np.float32(2.0 ** -70)  # E far beyond +-32
    for top_k, fetch_k in ((10, 40), (10, 10), (300, 300), (7, 1024)):
        rk, rd, rc = r = ref.search(po, Q, top_k, fetch_k, key_offset=1000)
        _same(s.search_flat_batch(Q, top_k, fetch_k), r, (top_k, fetch_k))
        assert rc[2] == 0 and (rk[1] == 1000 + np.arange(top_k)).all() and (top_k < 300 or (rk[0, 0::2] + 150 == rk[0, 1::2]).all())
    # fetch_k >= n: the exact top-k over Xq, restated without the screen
    for i in (0, 3, 4):
        d = np.array([po.dist_canon(Q[i], x) for x in ref.Xq], np.float32)
        order = np.lexsort((np.arange(300), flat_i8_ref.orderable(d)))
        assert (rk[i] == order[:7] + 1000).all() and (rd[i] == d[order[:7]]).all()
    s.close()


def test_cast_above_2_24(la, po):
    """integer-valued columns in +-{125, 126, 127}: the codes are the values (E = 0), |s| > 2^24 and odd sums exist, so the cast rounds"""
    rng = np.random.default_rng(3)
    base = rng.choice([-1.0, 1.0], 1536)
    X = np.tile(base, (300, 1)) * rng.choice([125.0, 126.0, 127.0], (300, 1536), p=[0.02, 0.03, 0.95])
    X[rng.random(X.shape) < 0.01] *= -1
    X[0] = 127 * base
    Q = np.stack([127 * base, -127 * base]).astype(np.float32)
    ref, s = flat_i8_ref.Index(X.astype(np.float32)), _handle(la, X.astype(np.float32))
    sc = ref.c32 @ Q[0].astype(np.int32)
    assert (ref.c == X).all() and np.abs(sc).min() > 2 ** 24 and (sc.astype(np.float32).astype(np.int64) != sc).any()
    _same(s.search_flat_batch(Q, 10, 20), ref.search(po, Q, 10, 20), "saturated")
    s.close()


@pytest.mark.parametrize("name", ["3 percent, stray bits", "fewer than top_k", "none", "bitmap and removals"])
def test_bitmap_and_removals(la, po, cases, name):
    X, ref, s, Q = cases(768, 1500, True)
    n, removed = 1500, ()
    bm = np.zeros(n // 8 + 9, np.uint8)  # 9 bytes behind ceil(n / 8)
    bits = np.random.default_rng(11).random(n) < {"fewer than top_k": 0.004, "none": 0.0}.get(name, 0.03)
    bm[:(n + 7) // 8] = np.packbits(bits, bitorder="little")
    bm[(n + 7) // 8 - 1] |= 0xF0  # n % 8 == 4: stray bits behind n in the last byte, and whole stray bytes
    bm[(n + 7) // 8:] = 0xFF
    if "removals" in name:  # a handle of its own: removing changes it
        s = _handle(la, X)
        removed = [int(i) for i in np.flatnonzero(bits)[::3]] + [0, 1499]
        s.remove(np.array(sorted(set(removed)), np.uint64))
    r = ref.search(po, Q[:9], 10, 40, allow=bm, removed=removed)
    _same(s.search_flat_batch(Q[:9], 10, 40, allow=bm), r, name)
    assert (r[2] == {"fewer than top_k": bits.sum(), "none": 0}.get(name, 10)).all() and r[2].max() <= 10
    if "removals" in name:
        s.close()


def test_emission_path(la, po, monkeypatch):
    """70 000 rows, above the select plan's emission threshold (64 Ki): CandEmit; once more on the slab schedule: the same bits"""
    X, Q = synth(po, 70000, 128), synth(po, 8, 128, stream=1)
    ref, s = flat_i8_ref.Index(X), _handle(la, X)
    r = ref.search(po, Q, 10, 40)
    _same(s.search_flat_batch(Q, 10, 40), r, "emit")
    monkeypatch.setenv("LEANN_DEBUG_NO_EMIT", "1")
    la.lib().leann_debug_reload_env()
    _same(s.search_flat_batch(Q, 10, 40), r, "no_emit")
    s.close()


def test_distance_is_the_walks(cases):  # whatever key the int8 walk returns on the same handle: the same distance bits
    X, ref, s, Q = cases(768)
    fk, fd, fc = s.search_flat_batch(Q, 300, 300)
    wk, wd, wc = s.search_batch(Q, 64, 128)
    assert (fc == 300).all() and (wc == 64).all()
    for i in range(len(Q)):
        flat = dict(zip(fk[i].tolist(), fd[i].view(np.uint32).tolist()))
        assert [flat[k] for k in wk[i].tolist()] == wd[i].view(np.uint32).tolist()


def test_recall_of_the_screen(po, cases):
    """768-d, n = 1 500, clustered unit rows with four columns scaled up; top_k = 10, fetch_k = 40, 65 queries; recall@10 against
    po.exact_topk over the f32 rows.  Measured on the CPU from the reference alone: 0.9969 — what fetch_k = 1 024, the exact top-10
    over Xq, gives too; 0.9923 at fetch_k = 10; 0.986 and 0.991 for two other query seeds.  The margin of 0.02 covers another seed, not
    the device."""
    X, ref, s, Q = cases(768, 1500, True)
    r = ref.search(po, Q, 10, 40)
    _same(s.search_flat_batch(Q, 10, 40), r, "recall")
    assert recall_at_k(r[0], po.exact_topk(X, Q, 10)) >= 0.9969 - 0.02


def test_refusals_name_the_way_out(la, po, cases):
    X, L = cases(96)[0], la.lib()
    f32 = _handle(la, X, la.RowType.F32)
    dF, dW = la.DeviceArray.from_host(po.synth_features(SEED, 64, 64, 1.0, 0, 0, 600)), la.DeviceArray.from_host(po.synth_weights(SEED, 64, 64))
    r, hb = C.c_void_p(), C.c_void_p()
    la._native.check(L.leann_recompute_create(dF.ptr, 600, 64, dW.ptr, 64, 0, 0, C.byref(r)))
    la._native.check(L.leann_recompute_build_index(r, 0, 8, 64, C.byref(hb)))
    comp = la.ShardedIndex.from_searchers([_handle(la, X), _handle(la, X, key_offset=300)], take_ownership=True).as_backend()
    for h, words in ((f32.to_rows(la.RowType.BF16), ("bf16 rows", "round the query")), (comp, ("composite handle", "leann_merge_topk_device")),
                     (la.BackendSearcher(hb, la.BackendType.Hnsw), ("recomputes its vectors", "leann_recompute_search_batch_device")),
                     (f32, ("f32 rows", "leann_backend_search_filtered_exact_batch"))):
        with pytest.raises(la.LeannError) as e:
            h.search_flat_batch(np.zeros((2, h.dims()), np.float32), 2, 4)
        assert e.value.code == UNSUPPORTED and all(w in str(e.value) for w in words), str(e.value)
        h.close()
    L.leann_recompute_close(r)
