"""BM25 under an allow-bitmap, the parts that need no GPU: the numpy restatement of the definition (tests/bm25_masked_ref.py) against the
unmasked references it is built on, every case of tests/test_gpu_bm25_filtered.py held to the branch it exists for, and the argument
errors of the new entry points, which all come back before any device work."""
import ctypes as C

import numpy as np
import pytest

import bm25_masked_ref as mr
import hybrid_cases as hc

f32 = np.float32


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def test_bitmaps_pack_positions_as_the_abi_states_them():
    m = np.zeros(19, bool)
    m[[0, 9, 18]] = True
    b = mr.pack(m)
    assert b.tolist() == [1, 2, 4] and len(b) == mr.nbytes(19)  # bit i & 7 of byte i >> 3
    assert (mr.unpack(b, 19) == m).all()
    p = mr.with_pad_bits(b, 19)
    assert p.tolist() == [1, 2, 4 | 0xF8] and (mr.unpack(p, 19) == m).all()  # pad bits are ignored
    assert (mr.with_pad_bits(mr.pack(np.ones(16, bool)), 16) == 0xFF).all()  # no pad bits at a multiple of 8
    s = mr.strided([b, b], 5)
    assert s.tolist() == [1, 2, 4, 0xFF, 0xFF] * 2


def test_all_ones_mask_is_the_unmasked_reference():
    post = hc.corpus("small")
    ones = np.ones(post.n_docs, bool)
    for terms in hc.random_queries(np.random.default_rng(2), post, 12, 20, 1200) + [[]]:
        s = post.score_query(terms)
        for k in (1, 10, 1024):
            pos, sc, npos, mm = mr.search(post, terms, k, ones)
            ep, es = post.search(terms, k)
            assert (pos == ep).all() and (_bits(sc) == _bits(es)).all() and npos == int((s > 0).sum())
            assert (_bits(mm) == _bits([s.min(), s.max()])).all()
    c = hc.case("chunked")
    post = hc.post_of(c)
    ones = np.ones(post.n_docs, bool)
    for q in range(0, len(c["queries"]), 7):
        n = hc.n_list(c, q)
        for compat in (True, False):
            got = mr.hybrid(post, c["queries"][q], c["keys"][q, :n], c["dists"][q, :n], ones, 0.7, compat, c["fetch_k"], 10)
            exp = hc.expected(c, q, 0.7, compat, top_k=10)
            assert [i for i, _ in got] == [i for i, _ in exp] and (_bits([x for _, x in got]) == _bits([x for _, x in exp])).all(), q


def test_a_mask_restricts_positives_statistics_and_ties():
    post, best, tie, queries = hc.boundary_corpus(257)
    n = post.n_docs
    s = post.score_query([tie])
    assert _bits(s[n - 2]) == _bits(s[n - 1]) and s[n - 1] > 0  # equal scores: unmasked, the lower position wins
    assert post.search([tie], 1)[0][0] == n - 2
    pos, sc, npos, _ = mr.search(post, [tie], 1, mr.tie_mask(n))
    assert pos[0] == n - 1 and npos == 1
    # the best passage disallowed: the maximum moves, so every normalised BM25 term of the hybrid blend moves with it
    s = post.score_query([0, best, 0])
    m = mr.mask("no_best", n, s)
    assert not m[n - 1]
    _, _, _, mm = mr.search(post, [0, best, 0], 5, m)
    assert mm[1] < s.max() and mm[1] == s[:n - 1].max()
    # nothing allowed: the folds' identities
    pos, sc, npos, mm = mr.search(post, [0], 5, mr.mask("none", n))
    assert len(pos) == 0 and npos == 0 and mm == (f32(np.inf), f32(-np.inf))
    assert mr.hybrid(post, [0], [3, 4], [0.1, 0.2], mr.mask("none", n), 0.7, True, 50, 10) == []


# ---- every GPU case reaches its branch ----------------------------------------------------------------------------------------------
def test_sizes_sit_on_the_edges_they_are_for():
    assert {1, 7, 8, 9} <= set(mr.SIZES) and {31, 32, 33} <= set(mr.SIZES)          # byte and word edges of the bitmap
    assert {255, 257} <= set(mr.SIZES) and {hc.CAP, hc.CAP + 1, 2 * hc.CAP + 1} <= set(mr.SIZES)  # a workgroup's rows, the sweep's ranges
    assert len(hc.sweep_ranges(2 * hc.CAP + 1)) == 3
    for n in mr.SIZES:
        post, best, tie, queries = hc.boundary_corpus(n)
        s = post.score_query([best])
        for name in mr.MASKS:
            m = mr.mask(name, n, s)
            assert m.shape == (n,)
            if name == "no_first_range":
                assert m.any() == (n > hc.CAP)
            if name == "no_best":
                assert not m[n - 1] and m.sum() == n - 1


def test_rising_corpus_still_overflows_under_its_masks():
    post = hc.rising_corpus(mr.RISING_N)
    for q, terms in enumerate(hc.RISING_QUERIES):
        m = mr.rising_mask(q)
        assert not m.all() and m[16384:].all()
        s = mr.restrict(post.score_query(list(terms)), m)
        for k in (1, 256, 1024):
            counts = hc.sweep_survivors(s, k)
            assert hc.overflows(counts) == (list(terms) in ([0], [0, 1], [0, 0])), (q, k, counts)
    assert len({mr.rising_mask(q).tobytes() for q in range(3)}) == 3  # a stride has different bitmaps to tell apart


def test_stride_case_spans_chunks_with_an_unaligned_stride():
    c = hc.case(mr.STRIDE_CASE["corpus"])
    assert len(c["queries"]) == mr.STRIDE_CASE["nq"] == 2 * hc.SLOTS + 5
    assert mr.STRIDE_CASE["stride"] % 4 and mr.STRIDE_CASE["stride"] >= mr.nbytes(hc.post_of(c).n_docs)
    masks = mr.stride_masks()
    assert not masks[64].any() and not masks[132].any() and masks[65].all()  # empty and full sets in chunks other than the first
    assert len({m.tobytes() for m in masks}) > 100


def test_large_hybrid_masks_change_what_the_issue_says_they_change():
    c = hc.case(mr.LARGE_CASE)
    post, masks = hc.post_of(c), mr.large_masks()
    assert c["fetch_k"] == 256 and 512 in c["top_ks"]
    moved = 0
    for q in (0, 2, 4, 5, 8, 10):
        n = hc.n_list(c, q)
        args = (post, c["queries"][q], c["keys"][q, :n], c["dists"][q, :n])
        masked = mr.hybrid(*args, masks[q], 0.7, True, 256, 512)
        plain = mr.hybrid(*args, np.ones(post.n_docs, bool), 0.7, True, 256, 512)
        if q == 5:  # nothing allowed, a full ANN list
            assert n == 256 and masked == [] and len(plain) == 256
            continue
        best = hc.positives(c, q)[0]
        assert not masks[q][best[0]] and best[1] == post.score_query(c["queries"][q]).max()  # the unmasked maximum is disallowed
        common = dict(plain)
        s = post.score_query(c["queries"][q])
        differs = any(k in common and _bits(sc) != _bits(common[k]) for k, sc in masked)
        assert differs == (s[masks[q]].max() != s.max()), q  # (equal scores are common in this corpus: a second passage may hold the maximum)
        moved += differs
        if q == 4:  # an empty ANN list: everything is injected, and the disallowed head of bm25_top no longer is
            out = [p for p, _ in hc.positives(c, q)[:mr.LARGE_INJECTED_OUT]]
            assert n == 0 and set(out) <= {k for k, _ in plain} and not set(out) & {k for k, _ in masked}
            assert len(masked) == 256  # the list is refilled from further down: injection never names a disallowed position
    assert moved >= 2


# ---- argument errors ----------------------------------------------------------------------------------------------------------------
def test_filtered_entry_points_exist_and_refuse_bad_arguments_without_a_gpu(la):
    L = la.lib()
    for name in ("leann_bm25_search_filtered_batch", "leann_bm25_search_filtered_batch_device", "leann_bm25_hybrid_rerank_filtered_device",
                 "leann_backend_filter_bitmap_device"):
        assert hasattr(L, name) and name in la._native.SIGNATURES
    u32p, f32p, u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    q_off, q_term, q_idf = np.array([0, 2], np.uint32), np.array([0, 1], np.uint32), np.array([1, 1], np.float32)
    ptrs = (q_off.ctypes.data_as(u32p), q_term.ctypes.data_as(u32p), q_idf.ctypes.data_as(f32p))
    out_u, out_f, bm = np.zeros(64, np.uint32), np.zeros(64, np.float32), np.zeros(8, np.uint8)
    o = (out_u.ctypes.data_as(u32p), out_f.ctypes.data_as(f32p), out_u.ctypes.data_as(u32p), None, None)
    z = None

    def err():
        return L.leann_last_error().decode()

    # a null bitmap with a stride, named before anything else
    assert L.leann_bm25_search_filtered_batch(None, 1, *ptrs, 4, None, 8, *o) == 1 and "allow_stride" in err() and "null" in err()
    assert L.leann_bm25_search_filtered_batch_device(None, 1, *ptrs, 4, None, 8, z, z, z, z, z, None) == 1 and "allow_stride" in err()
    assert L.leann_bm25_hybrid_rerank_filtered_device(None, 1, *ptrs, z, z, z, 50, 0.5, 1, 10, None, 8, z, z, z, None) == 1
    assert "allow_stride" in err() and "leann_bm25_hybrid_rerank_filtered_device" in err()
    # the twins' checks, under the new names
    allow = bm.ctypes.data_as(u8p)
    assert L.leann_bm25_search_filtered_batch(None, 1, *ptrs, 0, allow, 0, *o) == 1 and "top_k" in err()
    assert L.leann_bm25_search_filtered_batch(None, 1, *ptrs, 5000, allow, 0, *o) == 1 and "top_k" in err()
    assert L.leann_bm25_search_filtered_batch(None, 1, *ptrs, 4, allow, 0, *o) == 1 and "null handle" in err()
    assert "leann_bm25_search_filtered_batch:" in err()
    bad_idf = np.array([1, -1], np.float32)
    assert L.leann_bm25_search_filtered_batch(None, 1, ptrs[0], ptrs[1], bad_idf.ctypes.data_as(f32p), 4, allow, 0, *o) == 1 and "q_idf[1]" in err()
    assert L.leann_bm25_search_filtered_batch_device(None, 1, *ptrs, 4, None, 0, z, z, z, z, z, None) == 1 and "null handle" in err()
    assert L.leann_bm25_hybrid_rerank_filtered_device(None, 1, *ptrs, z, z, z, 300, 0.7, 1, 10, None, 0, z, z, z, None) == 1 and "fetch_k 300" in err()
    assert L.leann_bm25_hybrid_rerank_filtered_device(None, 1, *ptrs, z, z, z, 50, 1.5, 1, 10, None, 0, z, z, z, None) == 1 and "alpha" in err()
    assert L.leann_bm25_hybrid_rerank_filtered_device(None, 1, *ptrs, z, z, z, 50, 0.5, 1, 10, None, 0, z, z, z, None) == 1 and "null handle" in err()
    # the registered filter's bitmap
    p, n = C.c_void_p(), C.c_size_t(7)
    assert L.leann_backend_filter_bitmap_device(None, C.byref(p), C.byref(n)) == 1 and "null filter" in err()
    # the wrappers take the new arguments; None is the old call
    import inspect
    for fn in (la.Bm25Index.search_batch, la.Bm25Index.search_batch_device, la.Bm25Index.hybrid_rerank_device):
        sig = inspect.signature(fn).parameters
        assert sig["allow"].default is None and sig["allow_stride"].default == 0
    from leann_rs_amd.backend import Filter
    assert callable(Filter.device_bitmap)
    idx = la.Bm25Index(None, 100, np.array([0, 1], np.uint64))  # tables only: no device handle
    with pytest.raises(la.LeannError, match="allow-bitmap holds 3 bytes, 13 are needed"):
        idx.search_batch((q_off, np.array([0, 0], np.uint32), q_idf), 4, allow=np.zeros(3, np.uint8))
    idx._h = None
