"""CPU suite: PQ rows (csrc/scan_pq.hip): leann_pq_encode and leann_pq_query_lut against tests/pq_rows_ref.py byte for byte on inputs
whose ties are real, and the refusals of the host entry points."""
import ctypes as C

import numpy as np
import pytest

import pq_rows_ref as ref

SHAPES = [(4, 4), (36, 4), (100, 8)]  # one sub-space; M = 9; a ragged last sub-space (M = 13)
TOP = np.nextafter(np.float32(1), np.float32(0))  # 1 - 2^-24: the largest L below a power of two, w = rne(2^14 - 2^-10) = 2^14


def inputs(n, nq, dims, dsub, seed=0):
    """rows, queries and centroids of small integers: every distance and every L is exact, equidistant centroids are common; centroid
    1 repeats centroid 0 and 255 repeats 7 (ties go to the lower one).  Column 0 of every sub-space is 0 but for centroid 9, which is
    (TOP, 0, ..); row 0 sits on that centroid in every sub-space."""
    rng, M = np.random.default_rng(seed + dims), ref.shape(dims, dsub)[0]
    Cb = rng.integers(-3, 4, (M, 256, dsub)).astype(np.float32)
    Cb[:, :, 0] = 0
    Cb[:, 1], Cb[:, 255] = Cb[:, 0], Cb[:, 7]
    Cb[:, 9] = 0
    Cb[:, 9, 0] = TOP
    X = rng.integers(-3, 4, (n, dims)).astype(np.float32)
    X[0] = ref.codebooks(Cb, dims, dsub)[:, 9].reshape(-1)[:dims]
    return X, rng.integers(-8, 9, (nq, dims)).astype(np.float32), Cb


def edge_queries(dims, dsub):
    """a query that is not finite, an all-zero one, one whose max |L| is denormal (E = 1, entries on rounding ties), and the unit
    vectors of every sub-space's column 0, whose max |L| is TOP: w reaches 2^14 in every sub-space"""
    Q = np.zeros((4, dims), np.float32)
    Q[0, dims // 2] = np.inf
    Q[2] = (np.arange(dims) % 5 - 2) * 2.0 ** -140
    Q[3, ::dsub] = 1
    return Q


@pytest.mark.parametrize("dims, dsub", SHAPES)
def test_encode_equals_the_restatement(la, dims, dsub):
    X, _, Cb = inputs(37, 1, dims, dsub)
    X[1, 0], X[2, dims - 1], X[3, 1 % dims] = np.nan, np.inf, -np.inf  # what is not finite counts as 0
    codes = la.pq_encode(X, Cb, dsub)
    M, pitch = ref.shape(dims, dsub)
    assert codes.shape == (37, pitch) and (codes == ref.encode(X, Cb, dsub)).all() and (codes[:, M:] == 0).all()
    assert not np.isin(codes[:, :M], (1, 255)).any() and (codes[0, :M] == 9).all()  # duplicates lose to the lower index


@pytest.mark.parametrize("dims, dsub", SHAPES)
def test_query_tables_equal_the_restatement(la, dims, dsub):
    _, Q, Cb = inputs(1, 3, dims, dsub)
    for i, q in enumerate(np.concatenate([Q, edge_queries(dims, dsub)])):
        w, has = la.pq_query_lut(q, Cb, dsub)
        ww, whas = ref.query_lut(q, Cb, dsub)
        assert has == whas == (i != 3) and (w == ww).all()
        if i == 4:
            assert (w == 0).all()  # the all-zero query has tables, of zeros
        if i == 5:
            assert np.abs(w).max() <= 2 ** 13 and np.abs(w).max() > 0  # E = 1: 2^139 times a denormal
        if i == 6:
            assert (w[:, 9] == 2 ** 14).all() and np.abs(w.astype(np.int32)).max() == 2 ** 14


def test_refusals(la):
    L, u8p, f32p = la.lib(), C.POINTER(C.c_uint8), C.POINTER(C.c_float)
    X, Q, Cb = inputs(4, 1, 8, 8)
    out, lut, bad = np.zeros((4, 16), np.uint8), np.zeros((1, 256), np.int16), Cb.copy()
    bad[0, 3, 2] = np.nan
    p = lambda a, t=f32p: a.ctypes.data_as(t)
    for word, args in (("dims = 0", (p(X), 4, 0, 8, p(Cb), p(out, u8p))), ("dims = 4097", (p(X), 4, 4097, 8, p(Cb), p(out, u8p))),
                       ("dsub = 5", (p(X), 4, 8, 5, p(Cb), p(out, u8p))), ("null rows", (None, 4, 8, 8, p(Cb), p(out, u8p))),
                       ("null out", (p(X), 4, 8, 8, p(Cb), None)), ("null codebooks", (p(X), 4, 8, 8, None, p(out, u8p))),
                       ("codebooks hold", (p(X), 4, 8, 8, p(bad), p(out, u8p)))):
        assert L.leann_pq_encode(*args) == 1 and word in L.leann_last_error().decode(), word
    i16p = C.POINTER(C.c_int16)
    for word, args in (("null q", (None, 8, 8, p(Cb), p(lut, i16p))), ("dsub = 16", (p(Q), 8, 16, p(Cb), p(lut, i16p))),
                       ("codebooks hold", (p(Q), 8, 8, p(bad), p(lut, i16p)))):
        assert L.leann_pq_query_lut(*args) == 1 and word in L.leann_last_error().decode(), word
    with pytest.raises(la.LeannError, match="codebooks must be"):
        la.pq_encode(X, Cb[:, :, :4], 4)
    assert L.leann_pq_train(p(X), 4, 8, 8, 1, 0, p(Cb)) == 1 and "n = 4" in L.leann_last_error().decode()
    h = C.c_void_p()
    assert L.leann_pq_rows_from_host(p(X), 4, 8, None, 8, 0, 0, C.byref(h)) == 1 and "codebooks" in L.leann_last_error().decode()
    assert L.leann_pq_rows_from_host(p(X), 4, 8, p(Cb), 8, 0, 0, None) == 1 and "null out" in L.leann_last_error().decode()
    assert (L.leann_pq_rows_len(None), L.leann_pq_rows_pitch(None), L.leann_pq_rows_dsub(None)) == (0, 0, 0)
    if la.device_count() == 0:  # only the missing device stands in the way: never a CPU computation
        assert L.leann_pq_rows_from_host(p(X), 4, 8, p(Cb), 8, 0, 0, C.byref(h)) == 4 and "no CPU fallback" in L.leann_last_error().decode()
        assert L.leann_pq_train(p(np.zeros((256, 8), np.float32)), 256, 8, 8, 1, 0, p(Cb)) == 4 and "no CPU fallback" in L.leann_last_error().decode()
