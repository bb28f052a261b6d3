"""-m gpu: the device BM25 index (csrc/bm25.hip) — Bm25Scorer::search for batches, and the hybrid leg with the BM25 score vector kept
dense on the device — against oracle/bm25_oracle.py on small text corpora and against the numpy restatement tests/bm25_ref.py on a
Zipf corpus of 200 000 passages where most queries are positive on nearly every passage.  Positions and f32 bits are compared exactly,
for every query, everywhere."""
import json
import os
import subprocess

import numpy as np
import pytest

import bm25_oracle as bo
import bm25_ref
from util import synth

pytestmark = pytest.mark.gpu
f32 = np.float32
U64MAX = np.iinfo(np.uint64).max
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "leann-rs_amd", "host", "leann")

N_DOCS, N_TERMS, CORPUS_SEED, QUERY_SEED = 200_000, 20_000, 20250, 13


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _check_search(post, queries, got, top_k):
    """every query of a search_batch answer against bm25_ref; returns per-query positives and the ties seen inside the lists"""
    pos, sc, cnt, npos, mm = got
    ties, positives = 0, []
    for q, terms in enumerate(queries):
        s = post.score_query(terms)
        ep, es = post.search(terms, top_k, scores=s)
        P = int((s > 0).sum())
        positives.append(P)
        assert npos[q] == P and cnt[q] == len(ep) == min(P, top_k), q
        assert (pos[q, :cnt[q]] == ep).all(), q
        assert (_bits(sc[q, :cnt[q]]) == _bits(es)).all(), q
        assert (pos[q, cnt[q]:] == 0xFFFFFFFF).all() and np.isneginf(sc[q, cnt[q]:]).all(), q
        assert (_bits(mm[q]) == _bits([s.min(), s.max()])).all(), q  # over ALL passages: 0.0 unless every passage is positive
        ties += int((np.diff(_bits(es).astype(np.int64)) == 0).sum())
    return positives, ties


def _packed(post, queries):
    q_off = np.zeros(len(queries) + 1, np.uint32)
    q_off[1:] = np.cumsum([len(q) for q in queries])
    q_term = np.array([t for q in queries for t in q], np.uint32)
    q_idf = np.array([post.idf(t) for q in queries for t in q], np.float32)
    return q_off, q_term, q_idf


def _index(la, post):
    return la.Bm25Index.from_postings(post.n_docs, post.post_off, post.post_doc, post.post_tf, post.doc_len, post.avg_doc_len)


@pytest.fixture(scope="module")
def big(la, gpu):
    post = bm25_ref.synth_corpus(CORPUS_SEED, N_DOCS, N_TERMS)
    idx = _index(la, post)
    yield post, idx
    idx.close()


# ---- 1. small text corpora against the oracle ----------------------------------------------------------------------------------------
def test_small_text_corpora_match_the_oracle(la, gpu):
    words = "rust python kernel graph vector search index query gpu wave lds bank memory cache".split()
    rng = np.random.default_rng(3)
    docs = [" ".join(rng.choice(words, size=int(rng.integers(2, 25)))) for _ in range(400)] + ["", "a b c"]
    docs[7] = "onlyhere " + docs[7]
    oracle = bo.Bm25Scorer.build(docs)
    idx = la.Bm25Index.from_texts(docs)
    queries = ["rust rust kernel", "graph unknownword vector", "", "nothingmatches atall", "onlyhere", "gpu wave lds bank memory cache gpu",
               "rust python kernel graph vector search index query", "x y z"]
    for top_k in (3, 500):  # 500 > the number of positives of "onlyhere"
        pos, sc, cnt, npos, mm = idx.search_batch(queries, top_k)
        for q, text in enumerate(queries):
            exp = oracle.search(text, top_k)
            s = oracle.score_query(text)
            assert cnt[q] == len(exp) and npos[q] == int((s > 0).sum()), text
            assert [int(x) for x in pos[q, :cnt[q]]] == [i for i, _ in exp], text
            assert (_bits(sc[q, :cnt[q]]) == _bits([x for _, x in exp])).all(), text
            assert (_bits(mm[q]) == _bits([s.min(), s.max()])).all(), text
    assert cnt[2] == 0 and cnt[3] == 0 and cnt[4] == 1
    idx.close()


# ---- 2. the large corpus ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fetch_k", [15, 50, 250])
def test_large_corpus_search_matches_the_reference(la, big, fetch_k):
    post, idx = big
    queries = bm25_ref.synth_queries(QUERY_SEED, 64, N_TERMS)
    positives, ties = _check_search(post, queries, idx.search_batch(_packed(post, queries), fetch_k), fetch_k)
    print(f"fetch_k={fetch_k}: positives min {min(positives)} median {int(np.median(positives))} max {max(positives)}, ties in lists {ties}")
    assert max(positives) == N_DOCS  # a query with every passage positive: min_b moves off 0.0
    assert min(positives) < 512      # and one that the sparse call's stride would still hold
    assert sum(p > 512 for p in positives) > len(positives) // 2
    assert ties > 0                  # the stable order (score descending, position ascending) is exercised


def test_rising_scores_overflow_the_candidate_lists(la, gpu):
    """scores that rise with the position make every row a survivor of the threshold sweep: the lists overflow and the chunk is
    selected by the segment sorter instead — same answer"""
    n = 40_000
    tf = (np.arange(n) // 4 + 1).astype(np.uint32)  # groups of 4 equal scores: ties too
    post = bm25_ref.Postings(n, np.array([0, n, n + 3], np.uint64), np.concatenate([np.arange(n), [5, 6, 7]]).astype(np.uint32),
                             np.concatenate([tf, [1, 1, 1]]).astype(np.uint32), np.full(n, 50, np.uint32), 50.0)
    idx = _index(la, post)
    queries = [[0], [1], [0, 1], []]
    for k in (10, 700):
        _check_search(post, queries, idx.search_batch(_packed(post, queries), k), k)
    idx.close()


# ---- 3. hybrid end to end -----------------------------------------------------------------------------------------------------------
def _oracle_leg(so, keys, dists, dense, pos_top, alpha, compat, top_k):
    """searcher.rs:146-169: polarity, BM25-only hits of bm25_top appended with 0.0, hybrid_rerank over the dense vector, top_k cut"""
    vr = [(int(k), f32(d) if compat else f32(f32(1.0) - f32(d))) for k, d in zip(keys, dists)]
    have = {i for i, _ in vr}
    for p in pos_top:
        if int(p) not in have:
            vr.append((int(p), f32(0.0)))
    return so.hybrid_rerank(vr, dense, alpha)[:top_k]


def _check_leg(so, post, queries, lists, out, fetch_k, alpha, compat, top_k, dense_cache):
    keys, dists, counts = lists
    rk, rs, rc = (a.to_host() for a in out)
    for q, terms in enumerate(queries):
        if q not in dense_cache:
            s = post.score_query(terms)
            dense_cache[q] = (s, post.search(terms, fetch_k, scores=s)[0])
        dense, top = dense_cache[q]
        exp = _oracle_leg(so, keys[q, :counts[q]], dists[q, :counts[q]], dense, top, alpha, compat, top_k)
        assert rc[q] == len(exp), q
        assert [int(x) for x in rk[q, :rc[q]]] == [i for i, _ in exp], q
        assert (_bits(rs[q, :rc[q]]) == _bits([x for _, x in exp])).all(), q
        assert (rk[q, rc[q]:] == U64MAX).all(), q


def test_vamana_walk_then_device_bm25_rerank_end_to_end(la, po, big):
    import searcher_oracle as so
    post, idx = big
    n, d, R, k, L, nq = N_DOCS, 64, 32, 10, 64, 24
    fetch_k = 5 * k
    X = synth(po, n, d)
    Q = synth(po, nq, d, stream=1)
    dX = la.DeviceArray.from_host(X)
    s = la.BackendSearcher.build_device(la.BackendType.DiskAnn, dX.ptr, n, d, d, R, 64)
    g = s.graph_export()
    G = po.Graph.from_arrays(X, g["M"], g["M0"], g["max_level"], g["entry"], g["levels"], g["upper_off"], g["adj0"], g["adjU"])
    ok, od, oc, _ = G.search_batch(Q, fetch_k, L, 1, 4)
    dQ = la.DeviceArray.from_host(Q)
    dk, dd, dc = la.DeviceArray((nq, fetch_k), np.uint64), la.DeviceArray((nq, fetch_k), np.float32), la.DeviceArray(nq, np.uint32)
    s.search_batch_device(dQ.ptr, nq, fetch_k, L, dk.ptr, dd.ptr, dc.ptr)
    la.sync()
    gk, gd, gc = dk.to_host(), dd.to_host(), dc.to_host()
    assert (gk == ok).all() and (gd == od).all() and (gc == oc).all()
    queries = bm25_ref.synth_queries(QUERY_SEED + 1, nq, N_TERMS)
    queries[5] = []  # no known token at all
    # short and empty ANN lists (searcher.rs:139-143 zips whatever came back)
    gc = gc.copy()
    gc[1], gc[2] = 0, 7
    dc.upload(gc)
    packed, cache = _packed(post, queries), {}
    for compat in (True, False):
        for alpha in (0.0, 0.3, 0.7, 1.0):
            out = idx.hybrid_rerank_device(packed, dk, dd, dc, fetch_k, alpha, compat, k)
            _check_leg(so, post, queries, (ok, od, gc), out, fetch_k, alpha, compat, k, cache)
    s.close()


# ---- 4. slot reuse --------------------------------------------------------------------------------------------------------------------
def test_slots_are_clean_when_reused(la, big):
    post, idx = big
    nq = 2 * idx.slots + 5
    queries = bm25_ref.synth_queries(QUERY_SEED + 2, nq, N_TERMS)
    _check_search(post, queries, idx.search_batch(_packed(post, queries), 20), 20)
    order = np.random.default_rng(1).permutation(nq)
    again = [queries[i] for i in order]  # other queries land in the slots the first run used
    _check_search(post, again, idx.search_batch(_packed(post, again), 20), 20)


# ---- 5. where the positives fit the stride, the sparse call and the new one agree ----------------------------------------------------
def test_sparse_and_dense_rerank_agree_when_the_stride_holds_all_positives(la, gpu):
    n_docs, n_terms, nq, fetch_k, top_k, stride = 5000, 4000, 48, 40, 8, 512
    post = bm25_ref.synth_corpus(5, n_docs, n_terms, len_lo=3, len_hi=9)
    rng = np.random.default_rng(6)
    queries = [[int(t) for t in rng.integers(200, n_terms, size=int(rng.integers(1, 5)))] for _ in range(nq)]  # rare terms: few positives
    idx = _index(la, post)
    packed = _packed(post, queries)
    pos, sc, cnt, npos, _ = idx.search_batch(packed, stride)
    assert npos.max() <= stride and npos.max() > 0
    keys = np.full((nq, fetch_k), U64MAX, np.uint64)
    dists = np.full((nq, fetch_k), np.inf, np.float32)
    counts = np.zeros(nq, np.uint32)
    for q in range(nq):
        c = fetch_k if q % 4 else int(rng.integers(0, fetch_k))
        chosen = list(pos[q, :min(int(cnt[q]), c // 2)]) + [int(x) for x in rng.choice(n_docs, size=c, replace=False)]
        uniq = list(dict.fromkeys(int(x) for x in chosen))[:c]
        keys[q, :len(uniq)], counts[q] = uniq, len(uniq)
        dists[q, :len(uniq)] = np.sort(rng.uniform(0.05, 1.2, size=len(uniq))).astype(np.float32)
    dk, dd, dc = la.DeviceArray.from_host(keys), la.DeviceArray.from_host(dists), la.DeviceArray.from_host(counts)
    dp, ds, dn = la.DeviceArray.from_host(pos), la.DeviceArray.from_host(sc), la.DeviceArray.from_host(cnt)
    for compat in (True, False):
        a = [x.to_host() for x in idx.hybrid_rerank_device(packed, dk, dd, dc, fetch_k, 0.6, compat, top_k)]
        ok, os_, oc = la.DeviceArray((nq, top_k), np.uint64), la.DeviceArray((nq, top_k), np.float32), la.DeviceArray(nq, np.uint32)
        la._native.check(la.lib().leann_hybrid_rerank_device(dk.ptr, dd.ptr, dc.ptr, nq, fetch_k, dp.ptr, ds.ptr, dn.ptr, stride, n_docs, 0.6,
                                                             1 if compat else 0, top_k, ok.ptr, os_.ptr, oc.ptr, None))
        la.sync()
        assert (a[0] == ok.to_host()).all() and (_bits(a[1]) == _bits(os_.to_host())).all() and (a[2] == oc.to_host()).all()
    idx.close()


# ---- 6. the lists of a sharded handle ----------------------------------------------------------------------------------------------------
def test_sharded_lists_rerank_through_the_bm25_handle(la, po, gpu):
    import searcher_oracle as so
    n, d, M, k, nq = 6016, 64, 16, 6, 20
    fetch_k = 5 * k
    post = bm25_ref.synth_corpus(8, n, 1500, len_lo=10, len_hi=30)
    idx = _index(la, post)
    X = synth(po, n, d)
    Q = synth(po, nq, d, stream=1)
    lows = [0, 3008, n]  # interior boundaries are multiples of 64
    parts = [la.DeviceArray.from_host(X[lows[g]:lows[g + 1]]) for g in range(2)]
    sh = la.ShardedIndex.build_device(la.BackendType.Hnsw, [p.ptr for p in parts], [lows[g + 1] - lows[g] for g in range(2)], d, d, M, 48,
                                      [0, 0], keep=parts)  # device list "0,0": two shards on one device
    dQ = la.DeviceArray.from_host(Q)
    dk, dd, dc = la.DeviceArray((nq, fetch_k), np.uint64), la.DeviceArray((nq, fetch_k), np.float32), la.DeviceArray(nq, np.uint32)
    sh.search_batch_device(dQ.ptr, nq, fetch_k, 64, dk.ptr, dd.ptr, dc.ptr)
    la.sync()
    lists = (dk.to_host(), dd.to_host(), dc.to_host())
    assert lists[0][lists[0] != U64MAX].max() >= lows[1]  # global keys from the second shard are in the lists
    queries = bm25_ref.synth_queries(9, nq, 1500)
    cache = {}
    for compat in (True, False):
        out = idx.hybrid_rerank_device(_packed(post, queries), dk, dd, dc, fetch_k, 0.7, compat, k)
        _check_leg(so, post, queries, lists, out, fetch_k, 0.7, compat, k, cache)
    idx.close()


# ---- 7. CLI ------------------------------------------------------------------------------------------------------------------------------
def test_cli_device_and_host_bm25_print_the_same(tmp_path, gpu):
    topics = ["rust ownership borrow checker lifetimes", "python asyncio event loop coroutine", "vector database embedding search",
              "graph traversal beam hnsw neighbours", "gpu kernel wavefront lds bandwidth", "bm25 ranking term frequency"]
    docs = [dict(id=str(i + 1), text=f"passage {i} about {topics[i % 6]} number {i * 7919 % 1000}", metadata=dict(lines=i)) for i in range(600)]
    (tmp_path / "docs.jsonl").write_text("\n".join(json.dumps(x) for x in docs))
    r = subprocess.run([EXE, "build", "--index-dir", str(tmp_path / "idx"), "--passages-jsonl", str(tmp_path / "docs.jsonl"), "--dimensions", "96",
                        "--graph-degree", "16", "--complexity", "64"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for polarity in ("true", "false"):
        for query in ("bm25 ranking frequency", "passage", "lifetimes gpu", "nothingmatches"):
            outs = []
            for where in ("device", "host"):
                r = subprocess.run([EXE, "search", query, "-i", str(tmp_path / "idx"), "--top-k", "7", "--format", "json", "--hybrid",
                                    "--compat-polarity", polarity, "--bm25", where], capture_output=True, text=True,
                                   env=dict(os.environ, LEANN_LOG="debug"))
                assert r.returncode == 0, r.stderr
                assert f"BM25 scored on the {where}" in r.stderr, r.stderr  # the path that was asked for is the path that ran
                outs.append(r.stdout)
            assert outs[0] == outs[1] and len(json.loads(outs[0])) == 7, (polarity, query)
    # alpha outside [0, 1] (and NaN): the reference takes any f32 (searcher.rs:57-59, bm25.rs:163); the device call does not, so the
    # default path scores such a query on the host — the parent's arithmetic — and answers as `--bm25 host` does
    for alpha in ("1.5", "-0.25", "nan"):
        outs = []
        for where in ("device", "host"):
            r = subprocess.run([EXE, "search", "bm25 ranking frequency", "-i", str(tmp_path / "idx"), "--top-k", "7", "--format", "json", "--hybrid",
                                "--hybrid-alpha", alpha, "--bm25", where], capture_output=True, text=True, env=dict(os.environ, LEANN_LOG="debug"))
            assert r.returncode == 0, (alpha, r.stderr)
            assert "BM25 scored on the host" in r.stderr, (alpha, r.stderr)
            outs.append(r.stdout)
        assert outs[0] == outs[1] and outs[0].count('"id"') == 7, alpha  # (a NaN score is printed as the parent prints it: not JSON)
    r = subprocess.run([EXE, "search", "x", "-i", str(tmp_path / "idx"), "--bm25", "elsewhere"], capture_output=True, text=True)
    assert r.returncode != 0 and "--bm25" in r.stderr


def test_cli_batch_equals_query_by_query(tmp_path, gpu):
    """IndexSearcher::search_batch_with_options (`leann search --queries-file`): more queries than the handle has slots, one backend
    call + one device BM25 + rerank call, against search_with_options query by query — which is what the same flag does with
    `--bm25 host` — and against single `leann search` invocations"""
    topics = ["rust ownership borrow checker lifetimes", "python asyncio event loop coroutine", "vector database embedding search",
              "graph traversal beam hnsw neighbours", "gpu kernel wavefront lds bandwidth", "bm25 ranking term frequency"]
    docs = [dict(id=str(i + 1), text=f"passage {i} about {topics[i % 6]} number {i * 7919 % 1000}", metadata=dict(lines=i)) for i in range(600)]
    (tmp_path / "docs.jsonl").write_text("\n".join(json.dumps(x) for x in docs))
    r = subprocess.run([EXE, "build", "--index-dir", str(tmp_path / "idx"), "--passages-jsonl", str(tmp_path / "docs.jsonl"), "--dimensions", "96",
                        "--graph-degree", "16", "--complexity", "64"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    words = sorted({w for t in topics for w in t.split()}) + ["passage", "number", "unknownword", "17"]
    rng = np.random.default_rng(4)
    queries = [" ".join(rng.choice(words, size=int(rng.integers(1, 6)))) for _ in range(150)]  # > 2 x 64 slots
    queries[3] = "nothingmatches"
    (tmp_path / "queries.txt").write_text("\n".join(queries))
    common = ["-i", str(tmp_path / "idx"), "--top-k", "6", "--format", "json", "--hybrid", "--compat-polarity", "false"]
    env = dict(os.environ, LEANN_LOG="debug")
    outs = {}
    for where in ("device", "host"):
        r = subprocess.run([EXE, "search", "--queries-file", str(tmp_path / "queries.txt"), "--bm25", where, *common], capture_output=True,
                           text=True, env=env)
        assert r.returncode == 0, r.stderr
        outs[where] = json.loads(r.stdout)
        assert ("BM25 scored on the device (batch of 150)" in r.stderr) == (where == "device"), r.stderr[-2000:]
    assert len(outs["device"]) == 150 and all(len(x) == 6 for x in outs["device"])
    assert outs["device"] == outs["host"]
    for q in (0, 3, 77, 149):
        r = subprocess.run([EXE, "search", queries[q], "--bm25", "device", *common], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert json.loads(r.stdout) == outs["device"][q], q
    # with a post-filter the whole merged list is walked, not its first top_k entries
    r1 = subprocess.run([EXE, "search", "--queries-file", str(tmp_path / "queries.txt"), "--bm25", "device", "-f", "lines>300", *common],
                        capture_output=True, text=True)
    r2 = subprocess.run([EXE, "search", "--queries-file", str(tmp_path / "queries.txt"), "--bm25", "host", "-f", "lines>300", *common],
                        capture_output=True, text=True)
    assert r1.returncode == 0 and r2.returncode == 0 and r1.stdout == r2.stdout
    assert all(x["metadata"]["lines"] > 300 for res in json.loads(r1.stdout) for x in res)


def test_device_entry_and_term_check_on_a_live_handle(la, big):
    """leann_bm25_search_batch_device leaves the lists of leann_bm25_search_batch in HBM; a term id beyond the handle's vocabulary
    is refused by both before any device work"""
    post, idx = big
    queries = bm25_ref.synth_queries(QUERY_SEED + 3, idx.slots + 3, N_TERMS)
    packed = _packed(post, queries)
    host = idx.search_batch(packed, 30)
    dev = [a.to_host() for a in idx.search_batch_device(packed, 30)]
    for h, d in zip(host, dev):
        assert (h.view(np.uint32) == d.view(np.uint32)).all()
    _check_search(post, queries, dev, 30)
    bad = (np.array([0, 2], np.uint32), np.array([0, N_TERMS], np.uint32), np.array([1.0, 1.0], np.float32))
    for call in (lambda: idx.search_batch(bad, 5), lambda: idx.search_batch_device(bad, 5)):
        with pytest.raises(la.LeannError, match=f"q_term\\[1\\] = {N_TERMS} >= n_terms {N_TERMS}"):
            call()
    _check_search(post, queries[:3], idx.search_batch(_packed(post, queries[:3]), 5), 5)  # the refused calls left the slots clean
