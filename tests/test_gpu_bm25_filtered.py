"""-m gpu: the device BM25 search and its hybrid rerank under an allow-bitmap (leann_bm25_search_filtered_batch[_device],
leann_bm25_hybrid_rerank_filtered_device; csrc/bm25.hip: bm25_emit_masked_kernel, the segment sorter under a bitmap,
bm25_empty_allow_kernel) against the numpy restatement of their definition, tests/bm25_masked_ref.py.  Positions, f32 score bits,
counts, n_positive, min_max bits and the unused tails are compared for every query; tests/test_cpu_bm25_masked.py shows on the
references that each case takes the path it is for.  Score vectors are computed once per (corpus, query) and shared."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import bm25_masked_ref as mr
import bm25_ref
import hybrid_cases as hc
from test_gpu_bm25 import _index
from util import HipStreams, synth

pytestmark = pytest.mark.gpu
U64MAX = hc.U64MAX
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "leann-rs_amd", "host", "leann")


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _check_search(post, queries, members, got, top_k, scores=None):
    """a filtered search answer (pos, scores, counts, n_positive, min_max), every query under its own member array"""
    pos, sc, cnt, npos, mm = got
    assert pos.shape == sc.shape == (len(queries), top_k)
    for q, terms in enumerate(queries):
        s = post.score_query(terms) if scores is None else scores[q]
        ep, es, P, emm = mr.search(post, terms, top_k, members[q], scores=s)
        what = (q, terms, int(members[q].sum()))
        assert npos[q] == P and cnt[q] == len(ep) == min(P, top_k), what
        assert (pos[q, :cnt[q]] == ep).all(), what
        assert (_bits(sc[q, :cnt[q]]) == _bits(es)).all(), what
        assert (pos[q, cnt[q]:] == 0xFFFFFFFF).all() and np.isneginf(sc[q, cnt[q]:]).all(), what
        assert (_bits(mm[q]) == _bits(emm)).all(), (what, mm[q], emm)


def _check_hybrid(post, queries, lists, members, out, fetch_k, alpha, compat, top_k, scores):
    keys, dists, counts = lists
    rk, rs, rc = out
    assert rk.shape == rs.shape == (len(queries), top_k)
    for q, terms in enumerate(queries):
        n = min(int(counts[q]), fetch_k)
        exp = mr.hybrid(post, terms, keys[q, :n], dists[q, :n], members[q], alpha, compat, fetch_k, top_k, scores=scores[q])
        what = (q, alpha, compat, top_k)
        assert rc[q] == len(exp), (what, int(rc[q]), len(exp))
        assert [int(x) for x in rk[q, :rc[q]]] == [i for i, _ in exp], what
        assert (_bits(rs[q, :rc[q]]) == _bits([x for _, x in exp])).all(), what
        assert (rk[q, rc[q]:] == U64MAX).all() and np.isneginf(rs[q, rc[q]:]).all(), what


@functools.lru_cache(maxsize=None)
def _scores(corpus, terms):
    s = hc.corpus(corpus).score_query(list(terms))
    s.setflags(write=False)
    return s


def _case_scores(c):
    return [_scores(c["corpus"], tuple(t)) for t in c["queries"]]


# ---- 1. the byte and word edges of the bitmap, the boundaries of the sweep's ranges -----------------------------------------------------
@pytest.mark.parametrize("n", mr.SIZES)
def test_masked_search_at_bitmap_and_range_edges(la, gpu, n):
    post, best, tie, queries = hc.boundary_corpus(n)
    queries = [list(q) for q in queries]
    scores = [post.score_query(q) for q in queries]
    idx = _index(la, post)
    nb = mr.nbytes(n)
    for name in mr.MASKS:
        if name == "no_best":  # the best passage of each query: one bitmap per query, at the smallest stride there is
            members = [mr.mask(name, n, s) for s in scores]
            allow, stride = mr.strided([mr.pack(m) for m in members], nb), nb
        else:
            members = [mr.mask(name, n)] * len(queries)
            allow, stride = mr.pack(members[0]), 0
        for k in mr.KS:
            _check_search(post, queries, members, idx.search_batch(hc.packed(post, queries), k, allow=allow, allow_stride=stride), k, scores)
        if stride == 0:  # whatever the pad bits of the last byte hold; the bitmap already in HBM
            padded = mr.with_pad_bits(allow, n)
            _check_search(post, queries, members, idx.search_batch(hc.packed(post, queries), 10, allow=padded), 10, scores)
            d_allow = la.DeviceArray.from_host(padded)
            got = [a.to_host() for a in idx.search_batch_device(hc.packed(post, queries), 10, allow=d_allow)]
            _check_search(post, queries, members, got, 10, scores)
    if n >= 2:  # equal scores on the last two rows: with the earlier one disallowed the later one is the answer
        members = [mr.tie_mask(n)] * len(queries)
        got = idx.search_batch(hc.packed(post, queries), 1, allow=mr.pack(members[0]))
        _check_search(post, queries, members, got, 1, scores)
        assert got[0][queries.index([tie]), 0] == n - 1
    idx.close()


# ---- 2. the overflow path: the segment sorter under a bitmap --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rising(la, gpu):
    idx = _index(la, hc.rising_corpus(mr.RISING_N))
    yield idx
    idx.close()


def test_rising_scores_overflow_under_one_bitmap_and_under_a_stride(la, rising):
    post = hc.rising_corpus(mr.RISING_N)
    queries = [list(q) for q in hc.RISING_QUERIES]
    scores = [post.score_query(q) for q in queries]
    packed = hc.packed(post, queries)
    stride = mr.nbytes(mr.RISING_N) + 1
    for k in (1, 256, 1024):
        members = [mr.rising_mask(0)] * len(queries)
        _check_search(post, queries, members, rising.search_batch(packed, k, allow=mr.pack(members[0])), k, scores)
        members = [mr.rising_mask(q) for q in range(len(queries))]
        allow = mr.strided([mr.pack(m) for m in members], stride)
        _check_search(post, queries, members, rising.search_batch(packed, k, allow=allow, allow_stride=stride), k, scores)


def test_hybrid_after_the_masked_chunk_was_reselected(la, rising):
    c = hc.case("rising_hybrid")
    post, queries, scores = hc.post_of(c), c["queries"], _case_scores(c)
    lists = tuple(c[a] for a in ("keys", "dists", "counts"))
    d_lists = [la.DeviceArray.from_host(a) for a in lists]
    stride = mr.nbytes(post.n_docs) + 2
    members = [mr.rising_mask(q) for q in range(len(queries))]
    d_allow = la.DeviceArray.from_host(mr.strided([mr.pack(m) for m in members], stride))
    for compat in (True, False):
        out = rising.hybrid_rerank_device(hc.packed(post, queries), *d_lists, c["fetch_k"], 0.7, compat, 20, allow=d_allow, allow_stride=stride)
        _check_hybrid(post, queries, lists, members, [a.to_host() for a in out], c["fetch_k"], 0.7, compat, 20, scores)


# ---- 3. strides and chunks ----------------------------------------------------------------------------------------------------------
def test_per_query_bitmaps_across_chunks_and_again_permuted(la, gpu):
    c = hc.case(mr.STRIDE_CASE["corpus"])
    post, stride, nq = hc.post_of(c), mr.STRIDE_CASE["stride"], mr.STRIDE_CASE["nq"]
    idx = _index(la, post)
    assert idx.slots == hc.SLOTS and nq == 2 * idx.slots + 5 and stride % 4
    all_scores, all_members = _case_scores(c), mr.stride_masks()
    for order in (np.arange(nq), np.random.default_rng(1).permutation(nq)):  # permuted: other bitmaps at the chunk offsets q0 > 0
        queries = [c["queries"][i] for i in order]
        members, scores = [all_members[i] for i in order], [all_scores[i] for i in order]
        lists = tuple(c[a][order] for a in ("keys", "dists", "counts"))
        allow = mr.strided([mr.pack(m) for m in members], stride)
        packed = hc.packed(post, queries)
        _check_search(post, queries, members, idx.search_batch(packed, 10, allow=allow, allow_stride=stride), 10, scores)
        d_lists = [la.DeviceArray.from_host(a) for a in lists]
        for compat in (True, False):
            out = idx.hybrid_rerank_device(packed, *d_lists, c["fetch_k"], 0.7, compat, 10, allow=allow, allow_stride=stride)
            _check_hybrid(post, queries, lists, members, [a.to_host() for a in out], c["fetch_k"], 0.7, compat, 10, scores)
    idx.close()


# ---- 4. hybrid: fetch_k 256, top_k up to 512 ------------------------------------------------------------------------------------------
def test_hybrid_under_masks_that_move_the_maximum_and_the_injection(la, gpu):
    c = hc.case(mr.LARGE_CASE)
    post, queries, scores, members = hc.post_of(c), c["queries"], _case_scores(c), mr.large_masks()
    idx = _index(la, post)
    lists = tuple(c[a] for a in ("keys", "dists", "counts"))
    d_lists = [la.DeviceArray.from_host(a) for a in lists]
    stride = mr.nbytes(post.n_docs)
    allow = mr.strided([mr.pack(m) for m in members], stride)
    packed = hc.packed(post, queries)
    plain = [a.to_host() for a in idx.hybrid_rerank_device(packed, *d_lists, c["fetch_k"], 0.7, True, 512)]
    for top_k in (51, 512):
        for compat in (True, False):
            for alpha in (0.0, 0.7):
                out = [a.to_host() for a in idx.hybrid_rerank_device(packed, *d_lists, c["fetch_k"], alpha, compat, top_k, allow=allow,
                                                                     allow_stride=stride)]
                _check_hybrid(post, queries, lists, members, out, c["fetch_k"], alpha, compat, top_k, scores)
                if top_k == 512 and compat and alpha == 0.7:
                    assert out[2][5] == 0 and plain[2][5] == 256  # nothing allowed: nothing returned, whatever the ANN list holds
                    assert (_bits(out[1][0, :50]) != _bits(plain[1][0, :50])).any()  # the maximum moved: other bits than the unmasked call's
                    gone = [p for p, _ in hc.positives(c, 4)[:mr.LARGE_INJECTED_OUT]]
                    assert np.isin(gone, plain[0][4]).all() and not np.isin(gone, out[0][4]).any()
    idx.close()


# ---- 5. no bitmap: the existing calls -------------------------------------------------------------------------------------------------
def test_null_bitmap_is_the_unfiltered_call(la, gpu):
    c = hc.case("chunked")
    post = hc.post_of(c)
    idx = _index(la, post)
    nq, fetch_k = len(c["queries"]), c["fetch_k"]
    q_off, q_term, q_idf = hc.packed(post, c["queries"])
    import ctypes as C
    u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    q = (idx._h, nq, q_off.ctypes.data_as(u32p), q_term.ctypes.data_as(u32p), q_idf.ctypes.data_as(f32p))
    L = la.lib()
    old = idx.search_batch((q_off, q_term, q_idf), 10)
    new = (np.zeros((nq, 10), np.uint32), np.zeros((nq, 10), np.float32), np.zeros(nq, np.uint32), np.zeros(nq, np.uint32),
           np.zeros((nq, 2), np.float32))
    la._native.check(L.leann_bm25_search_filtered_batch(*q, 10, None, 0, new[0].ctypes.data_as(u32p), new[1].ctypes.data_as(f32p),
                                                        new[2].ctypes.data_as(u32p), new[3].ctypes.data_as(u32p), new[4].ctypes.data_as(f32p)))
    d_old = idx.search_batch_device((q_off, q_term, q_idf), 10)
    d_new = [la.DeviceArray(a.shape, a.dtype) for a in new]
    la._native.check(L.leann_bm25_search_filtered_batch_device(*q, 10, None, 0, *[a.ptr for a in d_new], None))
    for a, b, d1, d2 in zip(old, new, d_old, d_new):
        assert a.tobytes() == b.tobytes() == d1.to_host().tobytes() == d2.to_host().tobytes()
    d_lists = [la.DeviceArray.from_host(c[a]) for a in ("keys", "dists", "counts")]
    h_old = idx.hybrid_rerank_device((q_off, q_term, q_idf), *d_lists, fetch_k, 0.7, True, 10)
    h_new = (la.DeviceArray((nq, 10), np.uint64), la.DeviceArray((nq, 10), np.float32), la.DeviceArray(nq, np.uint32))
    la._native.check(L.leann_bm25_hybrid_rerank_filtered_device(*q, *[a.ptr for a in d_lists], fetch_k, 0.7, 1, 10, None, 0,
                                                                *[a.ptr for a in h_new], None))
    for a, b in zip(h_old, h_new):
        assert a.to_host().tobytes() == b.to_host().tobytes()
    # the stride is checked against the handle's bitmap length before any device work
    d_allow = la.DeviceArray.from_host(np.full(mr.nbytes(post.n_docs), 0xFF, np.uint8))
    with pytest.raises(la.LeannError, match="allow_stride 5 is smaller than the 376-byte bitmap"):
        idx.search_batch_device((q_off, q_term, q_idf), 10, allow=d_allow, allow_stride=5)
    with pytest.raises(la.LeannError, match="allow_stride 375 is smaller"):
        idx.hybrid_rerank_device((q_off, q_term, q_idf), *d_lists, fetch_k, 0.7, True, 10, allow=d_allow, allow_stride=375)
    with pytest.raises(la.LeannError, match="allow_stride 1 is smaller"):
        idx.search_batch((q_off, q_term, q_idf), 10, allow=np.full(nq * 376, 0xFF, np.uint8), allow_stride=1)
    _check_search(post, c["queries"][:3], [np.ones(post.n_docs, bool)] * 3, idx.search_batch(hc.packed(post, c["queries"][:3]), 5,
                                                                                              allow=d_allow), 5)  # the slots are clean
    idx.close()


# ---- 6. a caller's stream: the bitmap is written by leann_meta_eval_device, the BM25 call is queued behind it -------------------------
def test_filtered_bm25_behind_meta_eval_on_a_callers_stream(la, gpu):
    post = hc.corpus("stream")
    n = post.n_docs
    idx = _index(la, post)
    recs = [dict(lines=int(i * 7919 % 1000)) for i in range(n)]
    m = la.MetaColumns.from_records(recs, ["lines"])
    member = np.array([r["lines"] > 600 for r in recs])
    queries = hc.random_queries(np.random.default_rng(5), post, hc.SLOTS + 6, 3, 600)
    packed = hc.packed(post, queries)
    poison = np.full(mr.nbytes(n), 0xAB, np.uint8)  # what an unordered read of the bitmap would see
    with HipStreams(la, 1) as st:
        d_bm = la.DeviceArray.from_host(poison)
        la.sync()
        m.eval_device("lines>600", d_bm.ptr, None, None, st[0])  # enqueued; the call below is ordered behind it on the same stream
        got = [a.to_host() for a in idx.search_batch_device(packed, 50, stream=st[0], allow=d_bm)]
        assert (mr.unpack(d_bm.to_host(), n) == member).all()
    _check_search(post, queries, [member] * len(queries), got, 50)
    m.close()
    idx.close()


# ---- 7. end to end: removals, a registered all-ones filter, the filtered walk, the filtered rerank ------------------------------------
def test_removed_rows_never_come_back_through_the_filtered_rerank(la, po, gpu):
    n, d, M, top_k, ef, nq = 2048, 64, 16, 10, 64, 24
    fetch_k = 5 * top_k
    post = bm25_ref.synth_corpus(61, n, 300, len_lo=5, len_hi=15)
    idx = _index(la, post)
    X, Q = synth(po, n, d), synth(po, nq, d, stream=1)
    dX = la.DeviceArray.from_host(X)
    s = la.BackendSearcher.build_device(la.BackendType.Hnsw, dX.ptr, n, d, d, M, 64)
    rng = np.random.default_rng(8)
    queries = hc.random_queries(rng, post, nq, 20, 900)
    scores = [post.score_query(q) for q in queries]
    removed = rng.random(n) < 0.1
    for q in range(0, nq, 2):  # the top BM25 hits of every other query are removed: they would have been injected
        removed[post.search(queries[q], 3, scores=scores[q])[0].astype(np.int64)] = True
    assert s.remove(np.flatnonzero(removed).astype(np.uint64)) == removed.sum()
    g = s.graph_export()  # (repairs are pending: the lists still name removed rows, the walk passes through them under the live mask)
    G = po.Graph.from_arrays(X, M, 2 * M, g["max_level"], g["entry"], g["levels"], g["upper_off"], g["adj0"], g["adjU"])
    live = ~removed
    flt = s.register_filter(np.full(mr.nbytes(n), 0xFF, np.uint8))  # all ones: leann_backend_filter_create ANDs the live mask
    assert flt.count() == live.sum()
    lists = s.search_filter_batch(Q, fetch_k, ef, flt, "walk")
    ok, od, oc, _ = G.search_filtered_batch(Q, fetch_k, ef, mr.pack(live), 0, 4)  # the oracle's walk of the same graph under the live mask
    assert (lists[0] == ok).all() and (_bits(lists[1]) == _bits(od)).all() and (lists[2] == oc).all()
    d_allow, n_pos = flt.device_bitmap()
    assert n_pos == n and d_allow
    d_lists = [la.DeviceArray.from_host(a) for a in (ok, od, oc)]
    for compat in (True, False):
        out = [a.to_host() for a in idx.hybrid_rerank_device(hc.packed(post, queries), *d_lists, fetch_k, 0.7, compat, top_k, allow=d_allow)]
        _check_hybrid(post, queries, (ok, od, oc), [live] * nq, out, fetch_k, 0.7, compat, top_k, scores)
        keys = out[0][out[0] != U64MAX].astype(np.int64)
        assert not removed[keys].any() and (out[2] == top_k).all()
    plain = idx.hybrid_rerank_device(hc.packed(post, queries), *d_lists, fetch_k, 0.7, True, 2 * fetch_k)[0].to_host()
    assert removed[plain[plain != U64MAX].astype(np.int64)].any()  # the unfiltered rerank does inject removed positions
    flt.close()
    s.close()
    idx.close()


# ---- 8. the C++ host: `leann search --hybrid --hybrid-filter inside` ----------------------------------------------------------------------
def test_cli_hybrid_filter_inside(tmp_path, gpu):
    """the 600 x 96 index of test_gpu_bm25.py's CLI tests, with removals: under --device-filter the rerank runs under the registered
    filter's bitmap, without a filter under the live positions; device and host BM25 print the same bytes, and the batch file path —
    one filtered search per 64 queries and one rerank call — the bytes of the single queries"""
    topics = ["rust ownership borrow checker lifetimes", "python asyncio event loop coroutine", "vector database embedding search",
              "graph traversal beam hnsw neighbours", "gpu kernel wavefront lds bandwidth", "bm25 ranking term frequency"]
    docs = [dict(id=str(i + 1), text=f"passage {i} about {topics[i % 6]} number {i * 7919 % 1000}", metadata=dict(lines=i)) for i in range(600)]
    (tmp_path / "docs.jsonl").write_text("\n".join(json.dumps(x) for x in docs))
    idx = str(tmp_path / "idx")
    env = dict(os.environ, LEANN_LOG="debug")

    def run(*args):
        return subprocess.run([EXE, *args], capture_output=True, text=True, env=env)

    r = run("build", "--index-dir", idx, "--passages-jsonl", str(tmp_path / "docs.jsonl"), "--dimensions", "96", "--graph-degree", "16",
            "--complexity", "64")
    assert r.returncode == 0, r.stderr
    common = ["-i", idx, "--top-k", "7", "--format", "json", "--hybrid", "--compat-polarity", "false"]
    query = "bm25 ranking frequency"
    r = run("search", query, *common)
    assert r.returncode == 0, r.stderr
    victims = [x["id"] for x in json.loads(r.stdout)[:3]]  # the best hybrid hits, top BM25 passages among them
    r = run("delete", idx, "--ids", ",".join(victims))
    assert r.returncode == 0, r.stderr
    flt = ["-f", "lines>450", "--device-filter"]
    # the default is `post`, byte for byte
    a, b = run("search", query, *common, *flt), run("search", query, *common, *flt, "--hybrid-filter", "post")
    assert a.returncode == 0 and b.returncode == 0 and a.stdout == b.stdout and "under the allow-bitmap" not in a.stderr
    for extra, passes in ((flt, lambda x: x["metadata"]["lines"] > 450), ([], lambda x: True)):
        outs = []
        for where in ("device", "host"):
            r = run("search", query, *common, *extra, "--hybrid-filter", "inside", "--bm25", where)
            assert r.returncode == 0, r.stderr
            assert f"BM25 scored on the {where}" in r.stderr and "hybrid rerank under the allow-bitmap" in r.stderr, r.stderr
            outs.append(r.stdout)
        res = json.loads(outs[0])
        assert outs[0] == outs[1] and len(res) == 7, extra
        assert all(passes(x) for x in res) and not {x["id"] for x in res} & set(victims), extra
    # the batch: more queries than one group of the filtered search, one rerank call
    words = sorted({w for t in topics for w in t.split()}) + ["passage", "number", "unknownword", "17"]
    rng = np.random.default_rng(4)
    queries = [" ".join(rng.choice(words, size=int(rng.integers(1, 6)))) for _ in range(70)]
    queries[3] = "nothingmatches"
    (tmp_path / "queries.txt").write_text("\n".join(queries))
    r = run("search", "--queries-file", str(tmp_path / "queries.txt"), *common, *flt, "--hybrid-filter", "inside")
    assert r.returncode == 0, r.stderr
    assert "BM25 scored on the device (batch of 70)" in r.stderr, r.stderr[-2000:]
    batch = json.loads(r.stdout)
    assert len(batch) == 70 and all(x["metadata"]["lines"] > 450 for res in batch for x in res)
    assert all(len(res) == 7 for q, res in enumerate(batch) if q != 3)
    h = run("search", "--queries-file", str(tmp_path / "queries.txt"), *common, *flt, "--hybrid-filter", "inside", "--bm25", "host")
    assert h.returncode == 0 and h.stdout == r.stdout
    for q in (0, 3, 65, 69):
        s = run("search", queries[q], *common, *flt, "--hybrid-filter", "inside")
        assert s.returncode == 0, s.stderr
        assert json.loads(s.stdout) == batch[q], q
    r = run("search", "x", "-i", idx, "--hybrid-filter", "sometimes")
    assert r.returncode != 0 and "--hybrid-filter" in r.stderr
