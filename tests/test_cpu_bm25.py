"""BM25 inverted index, the parts that need no GPU: the numpy restatement over CSR postings (tests/bm25_ref.py) against
oracle/bm25_oracle.py bit for bit, the postings / idf / search lists of Bm25Index.postings_from_texts and of the C++ Bm25Scorer
(host_selftest "bm25_index" mode, plain and AddressSanitizer builds) against the oracle on the reference's own corpora, and every
argument error of leann_bm25_create / leann_bm25_search_batch."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import bm25_oracle as bo
import bm25_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "leann-rs_amd", "host")
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_formulas.json")))
f32 = np.float32
WORDS = ("alpha beta gamma delta epsilon zeta eta theta iota kappa lambda mu nu xi omicron pi rho sigma tau upsilon phi chi psi omega "
         "rust python kernel graph vector search index query").split()


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _text_corpus(seed, n_docs):
    rng = np.random.default_rng(seed)
    p = bm25_ref.zipf_probabilities(len(WORDS), 1.1)
    return [" ".join(rng.choice(WORDS, size=int(rng.integers(3, 30)), p=p)) for _ in range(n_docs)]


def _text_queries(seed, n):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        toks = list(rng.choice(WORDS, size=int(rng.integers(1, 7))))
        if i % 4 == 0:
            toks.append(toks[0])  # a repeated token is added twice (bm25.rs:81)
        if i % 5 == 0:
            toks.insert(1, "unknownword")
        out.append(" ".join(toks))
    return out


def test_csr_restatement_equals_the_oracle_bit_for_bit():
    docs = _text_corpus(11, 300)
    oracle = bo.Bm25Scorer.build(docs)
    post, vocab = bm25_ref.from_texts(docs)
    mismatches = 0
    for q in _text_queries(12, 40):
        terms = [vocab[t] for t in bo.tokenize(q) if t in vocab]
        exp = oracle.score_query(q)
        got = post.score_query(terms)
        mismatches += int((_bits(exp) != _bits(got)).sum())
        pos, sc = post.search(terms, 25)
        top = oracle.search(q, 25)
        assert [int(x) for x in pos] == [i for i, _ in top]
        assert (_bits(sc) == _bits([s for _, s in top])).all()
    assert mismatches == 0


def test_synthetic_corpus_is_valid_csr():
    post = bm25_ref.synth_corpus(3, 2000, 500)
    assert int(post.post_off[-1]) == len(post.post_doc) == len(post.post_tf)
    assert int(post.post_tf.sum()) == int(post.doc_len.sum()) and (post.post_tf > 0).all()
    for t in range(post.n_terms):
        d = post.post_doc[int(post.post_off[t]):int(post.post_off[t + 1])]
        assert (np.diff(d.astype(np.int64)) > 0).all() and (d < post.n_docs).all()


def _gold_cases():
    cases = {k: dict(docs=v["docs"], queries=[v["query"], v["query"] + " " + v["query"], "zzzz " + v["query"]], top_k=3)
             for k, v in GOLD["bm25"].items()}
    cases["synthetic_text"] = dict(docs=_text_corpus(21, 120), queries=_text_queries(22, 12), top_k=10)
    return cases


def _expect(case):
    oracle = bo.Bm25Scorer.build(case["docs"])
    postings = {}
    for doc, tfm in enumerate(oracle.term_freqs):
        for t, c in tfm.items():
            postings.setdefault(t, []).append([doc, c])
    queries = []
    for q in case["queries"]:
        terms = [(t, bm25_ref.idf(oracle.num_docs, oracle.doc_freq[t])) for t in bo.tokenize(q) if oracle.doc_freq.get(t, 0)]
        queries.append(dict(terms=terms, scores=oracle.score_query(q), search=oracle.search(q, case["top_k"])))
    return postings, oracle.doc_lengths, oracle.avg_doc_len, queries


def test_python_index_tables_match_the_oracle(la):
    for name, case in _gold_cases().items():
        postings, doc_len, avg, queries = _expect(case)
        vocab, post_off, post_doc, post_tf, dl, a = la.Bm25Index.postings_from_texts(case["docs"])
        got = {t: [[int(post_doc[i]), int(post_tf[i])] for i in range(int(post_off[tid]), int(post_off[tid + 1]))] for t, tid in vocab.items()}
        assert got == postings, name
        assert dl.tolist() == doc_len and _bits(a) == _bits(avg), name
        idx = la.Bm25Index(None, len(case["docs"]), post_off, vocab)  # tables only: no device handle
        names = {tid: t for t, tid in vocab.items()}
        for q, exp in zip(case["queries"], queries):
            qt = idx.query_terms(q)
            assert [names[t] for t, _ in qt] == [t for t, _ in exp["terms"]], (name, q)
            assert (_bits([w for _, w in qt]) == _bits([w for _, w in exp["terms"]])).all(), (name, q)


def test_gold_scores_are_what_the_reference_recorded():
    for name, v in GOLD["bm25"].items():
        post, vocab = bm25_ref.from_texts(v["docs"])
        got = post.score_query([vocab[t] for t in bo.tokenize(v["query"]) if t in vocab])
        assert (_bits(got) == _bits(v["scores"])).all(), name


@pytest.mark.parametrize("exe", ["host_selftest", "host_selftest_asan"])
def test_cpp_scorer_tables_match_the_oracle(exe, tmp_path):
    path = os.path.join(HOST, exe)
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", ROOT, "leann-rs_amd/host/" + exe])
    cases = _gold_cases()
    p = tmp_path / "cases.json"
    p.write_text(json.dumps(dict(bm25_index=cases)))
    r = subprocess.run([path, str(p)], capture_output=True, text=True)
    assert r.returncode == 0 and "ERROR" not in r.stderr, r.stderr  # the asan build aborts with a report on any finding
    out = json.loads(r.stdout)["bm25_index"]
    for name, case in cases.items():
        postings, doc_len, avg, queries = _expect(case)
        got = out[name]
        assert got["postings"] == postings, name
        assert got["doc_len"] == doc_len and _bits(got["avg_doc_len"]) == _bits(avg), name
        for q, g, exp in zip(case["queries"], got["queries"], queries):
            assert [t for t, _ in g["terms"]] == [t for t, _ in exp["terms"]], (name, q)
            assert (_bits([w for _, w in g["terms"]]) == _bits([w for _, w in exp["terms"]])).all(), (name, q)
            assert (_bits(g["scores"]) == _bits(exp["scores"])).all(), (name, q)
            assert [i for i, _ in g["search"]] == [i for i, _ in exp["search"]], (name, q)
            assert (_bits([s for _, s in g["search"]]) == _bits([s for _, s in exp["search"]])).all(), (name, q)


# ---- argument errors: all of them come back before any device work, so also on a machine without a GPU ----------------------------
def _create(la, n_docs, off, doc, tf, dl, avg=10.0):
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    off, doc, tf, dl = np.array(off, np.uint64), np.array(doc, np.uint32), np.array(tf, np.uint32), np.array(dl, np.uint32)
    h = C.c_void_p()
    rc = la.lib().leann_bm25_create(n_docs, len(off) - 1, off.ctypes.data_as(u64p), doc.ctypes.data_as(u32p), tf.ctypes.data_as(u32p),
                                    dl.ctypes.data_as(u32p), avg, 0, C.byref(h))
    msg = la.lib().leann_last_error().decode()
    if rc == 0:
        la.lib().leann_bm25_close(h)
    return rc, msg


def test_create_rejects_bad_postings_without_a_gpu(la):
    good = dict(n_docs=4, off=[0, 2, 3], doc=[0, 2, 1], tf=[1, 2, 1], dl=[3, 4, 5, 6])
    rc, msg = _create(la, **good)
    if la.device_count() == 0:
        assert rc == 4 and "no CPU fallback" in msg  # valid input: only the missing device stands in the way
    else:
        assert rc == 0, msg
    for change, word in [(dict(off=[0, 3, 2]), "post_off not monotone"), (dict(off=[1, 2, 3]), "post_off[0]"),
                         (dict(doc=[0, 4, 1]), "post_doc[1] = 4 >= n_docs"), (dict(doc=[2, 0, 1]), "post_doc out of order"),
                         (dict(doc=[2, 2, 1]), "post_doc out of order"), (dict(tf=[1, 0, 1]), "post_tf[1] = 0"),
                         (dict(n_docs=0), "n_docs"), (dict(avg=0.0), "avg_doc_len"), (dict(avg=float("nan")), "avg_doc_len")]:
        rc, msg = _create(la, **{**good, **change})
        assert rc == 1 and word in msg, (change, msg)
    h = C.c_void_p()
    assert la.lib().leann_bm25_create(4, 2, None, None, None, None, 10.0, 0, C.byref(h)) == 1 and b"null" in la.lib().leann_last_error()
    with pytest.raises(la.LeannError, match="not at the posting count"):  # the ABI has no posting count of its own: the wrapper checks
        la.Bm25Index.from_postings(4, [0, 2, 4], [0, 2, 1], [1, 2, 1], [3, 4, 5, 6], 4.5)
    assert la.lib().leann_bm25_len(None) == 0 and la.lib().leann_bm25_slots(None) == 0
    la.lib().leann_bm25_close(None)


def test_search_rejects_bad_queries_without_a_gpu(la):
    L = la.lib()
    u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    out_u, out_f = np.zeros(64, np.uint32), np.zeros(64, np.float32)

    def search(q_off, q_term, q_idf, top_k=4, nq=None):
        q_off, q_term, q_idf = np.array(q_off, np.uint32), np.array(q_term, np.uint32), np.array(q_idf, np.float32)
        rc = L.leann_bm25_search_batch(None, len(q_off) - 1 if nq is None else nq, q_off.ctypes.data_as(u32p), q_term.ctypes.data_as(u32p),
                                       q_idf.ctypes.data_as(f32p), top_k, out_u.ctypes.data_as(u32p), out_f.ctypes.data_as(f32p),
                                       out_u.ctypes.data_as(u32p), None, None)
        return rc, L.leann_last_error().decode()

    for args, word in [(dict(q_off=[0, 2, 1], q_term=[0, 1], q_idf=[1, 1]), "q_off not monotone"),
                       (dict(q_off=[1, 2], q_term=[0, 1], q_idf=[1, 1]), "q_off[0]"),
                       (dict(q_off=[0, 2], q_term=[0, 1], q_idf=[1, -1]), "q_idf[1]"),
                       (dict(q_off=[0, 2], q_term=[0, 1], q_idf=[float("nan"), 1]), "q_idf[0]"),
                       (dict(q_off=[0, 2], q_term=[0, 1], q_idf=[1, 1], top_k=0), "top_k"),
                       (dict(q_off=[0, 2], q_term=[0, 1], q_idf=[1, 1], top_k=5000), "top_k"),
                       (dict(q_off=[0, 2], q_term=[0, 1], q_idf=[1, 1]), "null handle")]:
        rc, msg = search(**args)
        assert rc == 1 and word in msg, (args, msg)
    # a term id is checked against the handle's vocabulary; the same check, callable without a handle
    q_off, q_term, q_idf = np.array([0, 2], np.uint32), np.array([0, 7], np.uint32), np.array([1, 1], np.float32)
    ptrs = (q_off.ctypes.data_as(u32p), q_term.ctypes.data_as(u32p), q_idf.ctypes.data_as(f32p))
    assert L.leann_bm25_check_queries(7, 1, *ptrs) == 1 and b"q_term[1] = 7 >= n_terms 7" in L.leann_last_error()
    assert L.leann_bm25_check_queries(8, 1, *ptrs) == 0
    # the hybrid call: fetch_k and alpha
    z = None
    assert L.leann_bm25_hybrid_rerank_device(None, 1, *ptrs, z, z, z, 300, 0.7, 1, 10, z, z, z, None) == 1 and b"fetch_k 300" in L.leann_last_error()
    assert L.leann_bm25_hybrid_rerank_device(None, 1, *ptrs, z, z, z, 50, 1.5, 1, 10, z, z, z, None) == 1 and b"alpha" in L.leann_last_error()
    assert L.leann_bm25_hybrid_rerank_device(None, 1, *ptrs, z, z, z, 50, 0.5, 1, 10, z, z, z, None) == 1 and b"null handle" in L.leann_last_error()
