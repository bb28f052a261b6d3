"""Helper of the BM25 tests (not a test): Bm25Scorer::score_query / search (src/index/bm25.rs:77-122) restated in numpy float32 over CSR
postings — one vectorised read-add-write per query token, so a passage's contributions are added in query-token order exactly as the
reference's token loop adds them — and a seeded synthetic corpus: term ids from a Zipf law, passage lengths uniform in a range.
idf goes through libm's logf, as oracle/bm25_oracle.py does."""
import numpy as np

import bm25_oracle as bo

f32 = np.float32
K1, B = bo.K1, bo.B


def idf(num_docs, df):
    df = f32(df)
    ratio = f32(f32(f32(num_docs) - df) + f32(0.5)) / f32(df + f32(0.5))  # bm25.rs:88
    return bo.logf(f32(ratio + f32(1.0)))


class Postings:
    """CSR postings: post_off u64 [n_terms + 1], post_doc u32 ascending within a list, post_tf u32; doc_len u32, avg_doc_len f32"""

    def __init__(self, n_docs, post_off, post_doc, post_tf, doc_len, avg_doc_len):
        self.n_docs, self.post_off, self.post_doc, self.post_tf = n_docs, post_off, post_doc, post_tf
        self.doc_len, self.avg_doc_len = doc_len, f32(avg_doc_len)
        self.n_terms = len(post_off) - 1
        norm = (f32(1.0) - B) + B * (doc_len.astype(np.float32) / self.avg_doc_len)  # bm25.rs:97, every operation in f32
        assert norm.dtype == np.float32
        self.k1n = K1 * norm

    def df(self, term):
        return int(self.post_off[term + 1]) - int(self.post_off[term])

    def idf(self, term):
        return idf(self.n_docs, self.df(term))

    def query(self, terms):
        """[(term id, idf)] in token order for a list of KNOWN term ids"""
        return [(int(t), self.idf(int(t))) for t in terms]

    def score_query(self, terms):
        scores = np.zeros(self.n_docs, np.float32)
        for t in terms:
            lo, hi = int(self.post_off[t]), int(self.post_off[t + 1])
            if hi == lo:
                continue
            w = self.idf(t)
            doc = self.post_doc[lo:hi]
            tf = self.post_tf[lo:hi].astype(np.float32)
            contrib = (w * (tf * (K1 + f32(1.0)))) / (tf + self.k1n[doc])  # bm25.rs:100
            assert contrib.dtype == np.float32
            scores[doc] = scores[doc] + contrib  # a list holds a passage once: a plain gather-add-scatter
        return scores

    def search(self, terms, top_k, scores=None):
        """(positions, scores) of the positives, score descending, stable = position ascending (bm25.rs:109-122)"""
        s = self.score_query(terms) if scores is None else scores
        pos = np.flatnonzero(s > 0)
        order = np.argsort(-s[pos].astype(np.float64), kind="stable")[:top_k]
        return pos[order].astype(np.uint32), s[pos[order]]


def from_texts(texts):
    """the oracle's tables as CSR (term ids in order of first appearance); returns (Postings, vocab)"""
    sc = bo.Bm25Scorer.build(texts)
    vocab = {}
    for tfm in sc.term_freqs:
        for t in tfm:
            vocab.setdefault(t, len(vocab))
    lists = [[] for _ in vocab]
    for doc, tfm in enumerate(sc.term_freqs):
        for t, c in tfm.items():
            lists[vocab[t]].append((doc, c))
    post_off = np.zeros(len(lists) + 1, np.uint64)
    post_off[1:] = np.cumsum([len(x) for x in lists], dtype=np.uint64)
    post_doc = np.array([d for x in lists for d, _ in x], np.uint32)
    post_tf = np.array([c for x in lists for _, c in x], np.uint32)
    return Postings(len(texts), post_off, post_doc, post_tf, np.array(sc.doc_lengths, np.uint32), sc.avg_doc_len), vocab


def zipf_probabilities(n_terms, exponent):
    p = 1.0 / np.arange(1, n_terms + 1, dtype=np.float64) ** exponent
    return p / p.sum()


def synth_corpus(seed, n_docs, n_terms, exponent=1.1, len_lo=40, len_hi=120):
    """passage lengths uniform in [len_lo, len_hi], every token's term id drawn from Zipf(exponent) over n_terms"""
    rng = np.random.default_rng(seed)
    doc_len = rng.integers(len_lo, len_hi + 1, size=n_docs).astype(np.uint32)
    total = int(doc_len.sum())
    cdf = np.cumsum(zipf_probabilities(n_terms, exponent))
    cdf[-1] = 1.0
    term = np.searchsorted(cdf, rng.random(total), side="right").astype(np.uint64)
    doc = np.repeat(np.arange(n_docs, dtype=np.uint64), doc_len)
    pair, tf = np.unique(term * np.uint64(n_docs) + doc, return_counts=True)  # sorted by (term, doc): CSR order
    p_term = (pair // np.uint64(n_docs)).astype(np.int64)
    post_doc = (pair % np.uint64(n_docs)).astype(np.uint32)
    post_off = np.zeros(n_terms + 1, np.uint64)
    post_off[1:] = np.cumsum(np.bincount(p_term, minlength=n_terms), dtype=np.uint64)
    avg = f32(total) / f32(n_docs)
    return Postings(n_docs, post_off, post_doc, tf.astype(np.uint32), doc_len, avg)


def synth_queries(seed, n_queries, n_terms, exponent=1.1, lo=2, hi=8):
    """queries of lo..hi tokens drawn from the same law (repeats possible)"""
    rng = np.random.default_rng(seed)
    cdf = np.cumsum(zipf_probabilities(n_terms, exponent))
    cdf[-1] = 1.0
    return [np.searchsorted(cdf, rng.random(int(rng.integers(lo, hi + 1))), side="right").astype(np.int64).tolist() for _ in range(n_queries)]
