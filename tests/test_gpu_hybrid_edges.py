"""-m gpu: the hybrid rerank body (csrc/hybrid_rerank.cuh) behind both of its callers — the sparse leann_hybrid_rerank_device
(csrc/hybrid.hip) and the dense leann_bm25_hybrid_rerank_device (csrc/bm25.hip) — and the device BM25 search, at the sizes
test_gpu_hybrid.py and test_gpu_bm25.py leave out:
    a  merged lists of 257 to 512 entries (fetch_k up to 256, top_k up to 512): the second stride of every 256-thread loop
    b  arguments the code clamps or widens: counts > fetch_k, keys >= n_docs, a u64 key whose low word is an injected position,
       count > stride, fetch_k = top_k = 1
    c  the dense call over more queries than the handle has slots, and again with the queries permuted
    d  candidate lists exactly full and one entry over, for the search and for the dense call after the chunk was reselected
    e  corpora that end on, or one row past, a boundary of the sweep's row ranges, and corpora smaller than a workgroup
    f  the device BM25 calls queued on a caller's stream behind the search that produces their lists
The cases are tests/hybrid_cases.py's; tests/test_cpu_hybrid_cases.py shows on the references that each takes the path it is for.
Ids, f32 score bits, counts and the unused tails are compared for every query; expectations come from oracle/searcher_oracle.py and
tests/bm25_ref.py and are computed once per (case, query, alpha, polarity)."""
import functools

import numpy as np
import pytest

import hybrid_cases as hc
from test_gpu_bm25 import _check_search, _index
from util import HipStreams, synth

pytestmark = pytest.mark.gpu
U64MAX = hc.U64MAX


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _expected(name, q, alpha, compat, sparse):
    """(ids u64, score bits u32) of the whole merged list of query q, best first"""
    c = hc.case(name)
    if sparse and hc.n_sparse(c, q) == len(hc.positives(c, q)):
        return _expected(name, q, alpha, compat, False)  # the stride holds every positive: the same computation
    exp = hc.expected(c, q, alpha, compat, sparse=sparse)
    return np.array([i for i, _ in exp], np.uint64), _bits([s for _, s in exp])


def _assert_answer(got, want, top_k, what):
    """got: (keys [nq x top_k], scores, counts) on the host; want(q) -> (ids, score bits) of the whole merged list"""
    gk, gs, gc = got
    assert gk.shape == gs.shape == (len(gc), top_k)
    for q in range(len(gc)):
        ids, bits = want(q)
        n = min(len(ids), top_k)
        assert gc[q] == n, (what, q, int(gc[q]), n)
        assert (gk[q, :n] == ids[:n]).all(), (what, q)
        assert (_bits(gs[q, :n]) == bits[:n]).all(), (what, q)
        assert (gk[q, n:] == U64MAX).all() and np.isneginf(gs[q, n:]).all(), (what, q)


class _Lists:
    """a case's lists and sparse BM25 side in HBM"""

    def __init__(self, la, c, sparse=True):
        self.c, self.nq = c, len(c["queries"])
        self.keys, self.dists, self.counts = (la.DeviceArray.from_host(c[a]) for a in ("keys", "dists", "counts"))
        self.sparse = [la.DeviceArray.from_host(a) for a in hc.sparse_arrays(c)] if sparse else None
        self.packed = hc.packed(hc.post_of(c), c["queries"])


def _run_sparse(la, L, alpha, compat, top_k):
    c = L.c
    ok, os_, oc = la.DeviceArray((L.nq, top_k), np.uint64), la.DeviceArray((L.nq, top_k), np.float32), la.DeviceArray(L.nq, np.uint32)
    la._native.check(la.lib().leann_hybrid_rerank_device(L.keys.ptr, L.dists.ptr, L.counts.ptr, L.nq, c["fetch_k"], L.sparse[0].ptr,
                                                         L.sparse[1].ptr, L.sparse[2].ptr, c["stride"], hc.post_of(c).n_docs, alpha,
                                                         1 if compat else 0, top_k, ok.ptr, os_.ptr, oc.ptr, None))
    la.sync()
    return ok.to_host(), os_.to_host(), oc.to_host()


def _run_dense(idx, L, alpha, compat, top_k, stream=None):
    out = idx.hybrid_rerank_device(L.packed, L.keys, L.dists, L.counts, L.c["fetch_k"], alpha, compat, top_k, stream=stream)
    return tuple(a.to_host() for a in out)


def _both_calls(la, idx, name):
    """every top_k, polarity and alpha of a case through both calls; where the stride holds all positives of a query the two agree"""
    c = hc.case(name)
    L = _Lists(la, c)
    fits = np.array([len(hc.positives(c, q)) <= c["stride"] for q in range(L.nq)])
    assert fits.any()
    for top_k in c["top_ks"]:
        for compat in (True, False):
            for alpha in hc.ALPHAS:
                what = (name, top_k, compat, alpha)
                s = _run_sparse(la, L, alpha, compat, top_k)
                _assert_answer(s, lambda q: _expected(name, q, alpha, compat, True), top_k, ("sparse",) + what)
                d = _run_dense(idx, L, alpha, compat, top_k)
                _assert_answer(d, lambda q: _expected(name, q, alpha, compat, False), top_k, ("dense",) + what)
                assert (s[0][fits] == d[0][fits]).all() and (_bits(s[1][fits]) == _bits(d[1][fits])).all() and (s[2][fits] == d[2][fits]).all()


@pytest.fixture(scope="module")
def small(la, gpu):
    idx = _index(la, hc.corpus("small"))
    yield idx
    idx.close()


@pytest.fixture(scope="module")
def rising(la, gpu):
    made = {}

    def get(n):
        if n not in made:
            made[n] = _index(la, hc.rising_corpus(n))
        return made[n]

    yield get
    for idx in made.values():
        idx.close()


# ---- a. merged lists above 256 entries --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["large_m_128", "large_m_255", "large_m_256"])
def test_rerank_body_above_256_entries_through_both_calls(la, small, name):
    _both_calls(la, small, name)


# ---- b. clamps and widening -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["clamps", "ones"])
def test_clamped_and_widened_arguments(la, small, name):
    _both_calls(la, small, name)


# ---- c. more queries than slots ---------------------------------------------------------------------------------------------------------
def test_dense_rerank_across_chunks_and_again_permuted(la, gpu):
    c = hc.case("chunked")
    idx = _index(la, hc.post_of(c))
    nq, top_k = len(c["queries"]), c["top_ks"][0]
    assert idx.slots == hc.SLOTS and nq == 2 * idx.slots + 5
    L = _Lists(la, c, sparse=False)
    for compat in (True, False):
        _assert_answer(_run_dense(idx, L, 0.7, compat, top_k), lambda q: _expected("chunked", q, 0.7, compat, False), top_k, ("chunked", compat))
    order = np.random.default_rng(1).permutation(nq)  # other queries land in the slots, and in other chunks
    assert (order // idx.slots != np.arange(nq) // idx.slots).sum() > nq // 2
    P = _Lists(la, dict(c, queries=[c["queries"][i] for i in order], keys=c["keys"][order], dists=c["dists"][order], counts=c["counts"][order]),
               sparse=False)
    for compat in (True, False):
        _assert_answer(_run_dense(idx, P, 0.7, compat, top_k), lambda q: _expected("chunked", int(order[q]), 0.7, compat, False), top_k,
                       ("chunked, permuted", compat))
    idx.close()


# ---- d. candidate lists exactly full, and one entry over --------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [24576, 24577])
def test_search_with_lists_exactly_full_and_one_over(la, rising, n):
    post, idx = hc.rising_corpus(n), rising(n)
    queries = [list(q) for q in hc.RISING_QUERIES]
    for k in hc.RISING_KS:
        got = idx.search_batch(hc.packed(post, queries), k)
        positives, _ = _check_search(post, queries, got, k)
        assert positives[0] == n and got[4][0, 0] > 0  # every passage positive: the minimum of the score vector is not 0.0
        assert (got[0][0, :k] == np.arange(n - 1, n - 1 - k, -1)).all()  # rising scores: the last k positions, backwards


def test_dense_rerank_after_the_chunk_was_reselected(la, rising):
    c = hc.case("rising_hybrid")
    idx = rising(hc.post_of(c).n_docs)
    L = _Lists(la, c, sparse=False)  # every passage is positive: no stride holds that
    top_k = c["top_ks"][0]
    for compat in (True, False):
        for alpha in (0.0, 0.7):
            _assert_answer(_run_dense(idx, L, alpha, compat, top_k), lambda q: _expected("rising_hybrid", q, alpha, compat, False), top_k,
                           ("rising", compat, alpha))


# ---- e. range boundaries and tiny corpora -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", hc.BOUNDARY_SIZES)
def test_search_at_range_boundaries_and_below_one_workgroup(la, gpu, n):
    post, best, tie, queries = hc.boundary_corpus(n)
    queries = [list(q) for q in queries]
    idx = _index(la, post)
    for top_k in (1, 1024):
        got = idx.search_batch(hc.packed(post, queries), top_k)
        _check_search(post, queries, got, top_k)
        assert got[0][queries.index([best]), 0] == n - 1
        assert got[0][queries.index([tie]), 0] == max(n - 2, 0)
    idx.close()


# ---- f. a caller's stream ---------------------------------------------------------------------------------------------------------------
def test_device_bm25_calls_on_a_callers_stream_behind_the_search(la, po, gpu):
    """search_batch_device of a graph handle on a non-blocking stream and, with no synchronisation in between, the dense rerank of
    its lists and a BM25 search on the same stream: the bytes of the same three calls on the null stream.  (Not captured into a graph:
    the BM25 calls copy and synchronise inside, include/leann_backend.h.)"""
    n, d, m, fetch_k, top_k, ef, nq = 4000, 64, 16, 50, 10, 64, hc.SLOTS + 6
    post = hc.corpus("stream")
    assert post.n_docs == n
    idx = _index(la, post)
    X, Q = synth(po, n, d), synth(po, nq, d, stream=1)
    dX, dQ = la.DeviceArray.from_host(X), la.DeviceArray.from_host(Q)
    s = la.BackendSearcher.build_device(la.BackendType.Hnsw, dX.ptr, n, d, d, m, 64)
    queries = hc.random_queries(np.random.default_rng(5), post, nq, 3, 600)
    queries[hc.SLOTS + 2] = []
    packed = hc.packed(post, queries)

    def poisoned(shape, dtype):
        """a buffer filled with a pattern no answer holds: what an earlier call left cannot pass for this one's"""
        a = np.empty(shape, dtype)
        a.view(np.uint8)[...] = 0xAB
        return la.DeviceArray.from_host(a)

    def chain(stream):
        lists = poisoned((nq, fetch_k), np.uint64), poisoned((nq, fetch_k), np.float32), poisoned(nq, np.uint32)
        bm = (poisoned((nq, fetch_k), np.uint32), poisoned((nq, fetch_k), np.float32), poisoned(nq, np.uint32), poisoned(nq, np.uint32),
              poisoned((nq, 2), np.float32))
        la.sync()
        s.search_batch_device(dQ.ptr, nq, fetch_k, ef, lists[0].ptr, lists[1].ptr, lists[2].ptr, stream=stream)
        top = idx.hybrid_rerank_device(packed, *lists, fetch_k, 0.7, True, top_k, stream=stream)
        idx.search_batch_device(packed, fetch_k, stream=stream, out=bm)
        la.sync()
        return [a.to_host() for a in lists], [a.to_host() for a in top], [a.to_host() for a in bm]

    with HipStreams(la, 1) as st:
        on_stream = chain(st[0])
    serial = chain(None)
    for group_a, group_b, what in zip(on_stream, serial, ("lists", "reranked", "bm25 search")):
        for a, b in zip(group_a, group_b):
            assert a.tobytes() == b.tobytes(), what
    lists, top, bm = serial
    assert (lists[0][:, 0] != 0xABABABABABABABAB).all() and lists[2].max() == fetch_k
    c = dict(corpus="stream", fetch_k=fetch_k, stride=hc.MAX_FETCH, queries=queries, keys=lists[0], dists=lists[1], counts=lists[2])

    def want(q):
        exp = hc.expected(c, q, 0.7, True)
        return np.array([i for i, _ in exp], np.uint64), _bits([x for _, x in exp])

    _assert_answer(top, want, top_k, "behind the search, null stream")
    _check_search(post, queries, bm, fetch_k)
    s.close()
    idx.close()
