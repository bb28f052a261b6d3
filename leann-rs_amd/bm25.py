"""Bm25Index — the device-resident BM25 inverted index (csrc/bm25.hip) behind ctypes.

Tokenisation, the term dictionary and the idf of a query term are host work (strings, and libm's logf: src/index/bm25.rs:88,
:127-132); scoring, selection and the hybrid rerank run on the device, bit for bit the reference's f32 arithmetic."""
import ctypes as C
import ctypes.util
import re

import numpy as np

from . import _native as N
from .device import DeviceArray

_TOKEN = re.compile(r"[a-zA-Z0-9]+")
_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype = C.c_float
_libm.logf.argtypes = [C.c_float]
f32 = np.float32


def tokenize(text):
    """bm25.rs:127-132: [a-zA-Z0-9]+, lowercased, one-character tokens dropped"""
    return [m.group(0).lower() for m in _TOKEN.finditer(text) if len(m.group(0)) > 1]


def idf(num_docs, df):
    """bm25.rs:88 in f32, ln through libm's logf"""
    df = f32(df)
    ratio = f32(f32(f32(num_docs) - df) + f32(0.5)) / f32(df + f32(0.5))
    return f32(_libm.logf(float(f32(ratio + f32(1.0)))))


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class Bm25Index:
    def __init__(self, handle, n_docs, post_off, vocab=None):
        self._h = handle
        self.n_docs = int(n_docs)
        self.post_off = post_off
        self.n_terms = len(post_off) - 1
        self.vocab = vocab  # token -> term id (from_texts only)

    @classmethod
    def from_postings(cls, n_docs, post_off, post_doc, post_tf, doc_len, avg_doc_len, device=0, vocab=None):
        post_off = np.ascontiguousarray(post_off, np.uint64)
        post_doc = np.ascontiguousarray(post_doc, np.uint32)
        post_tf = np.ascontiguousarray(post_tf, np.uint32)
        doc_len = np.ascontiguousarray(doc_len, np.uint32)
        if post_off.ndim != 1 or len(post_off) < 1:
            raise N.LeannError(1, "Bm25Index.from_postings: post_off must hold n_terms + 1 offsets")
        if len(doc_len) != n_docs:
            raise N.LeannError(1, f"Bm25Index.from_postings: doc_len has {len(doc_len)} entries, n_docs is {n_docs}")
        if len(post_doc) != len(post_tf) or int(post_off[-1]) != len(post_doc):
            raise N.LeannError(1, f"Bm25Index.from_postings: post_off ends at {int(post_off[-1])}, not at the posting count "
                                  f"{len(post_doc)} (post_tf: {len(post_tf)})")
        h = C.c_void_p()
        N.check(N.lib().leann_bm25_create(n_docs, len(post_off) - 1, _p(post_off, C.c_uint64), _p(post_doc, C.c_uint32),
                                          _p(post_tf, C.c_uint32), _p(doc_len, C.c_uint32), float(f32(avg_doc_len)), device, C.byref(h)))
        return cls(h, n_docs, post_off, vocab)

    @staticmethod
    def postings_from_texts(texts):
        """Bm25Scorer::build (bm25.rs:33-74) as CSR: term ids in order of first appearance, passages ascending within a list.
        Returns (vocab, post_off, post_doc, post_tf, doc_len, avg_doc_len)."""
        vocab, lists, doc_len, total = {}, [], [], 0
        for doc, text in enumerate(texts):
            toks = tokenize(text)
            doc_len.append(len(toks))
            total += len(toks)
            tf = {}
            for t in toks:
                tf[t] = tf.get(t, 0) + 1
            for t, c in tf.items():
                tid = vocab.setdefault(t, len(vocab))
                if tid == len(lists):
                    lists.append([])
                lists[tid].append((doc, c))
        post_off = np.zeros(len(lists) + 1, np.uint64)
        post_off[1:] = np.cumsum([len(x) for x in lists], dtype=np.uint64)
        flat = [p for x in lists for p in x]
        post_doc = np.array([d for d, _ in flat], np.uint32)
        post_tf = np.array([c for _, c in flat], np.uint32)
        avg = f32(total) / f32(len(texts)) if len(texts) else f32(1.0)
        return vocab, post_off, post_doc, post_tf, np.array(doc_len, np.uint32), avg

    @classmethod
    def from_texts(cls, texts, device=0):
        vocab, post_off, post_doc, post_tf, doc_len, avg = cls.postings_from_texts(texts)
        return cls.from_postings(len(texts), post_off, post_doc, post_tf, doc_len, avg, device, vocab)

    def query_terms(self, text):
        """(term id, idf) of the query's known tokens, in token order (repeats kept, unknown tokens skipped: bm25.rs:81-90)"""
        if self.vocab is None:
            raise N.LeannError(1, "Bm25Index.query_terms: the index was made from postings, it has no term dictionary")
        out = []
        for t in tokenize(text):
            tid = self.vocab.get(t)
            if tid is None:
                continue
            out.append((tid, idf(self.n_docs, int(self.post_off[tid + 1]) - int(self.post_off[tid]))))
        return out

    def idf_of(self, term_ids):
        return np.array([idf(self.n_docs, int(self.post_off[t + 1]) - int(self.post_off[t])) for t in term_ids], np.float32)

    @staticmethod
    def pack_queries(queries):
        """list of [(term id, idf), ...] -> (q_off, q_term, q_idf)"""
        q_off = np.zeros(len(queries) + 1, np.uint32)
        q_off[1:] = np.cumsum([len(q) for q in queries], dtype=np.uint64)
        q_term = np.array([t for q in queries for t, _ in q], np.uint32)
        q_idf = np.array([w for q in queries for _, w in q], np.float32)
        return q_off, q_term, q_idf

    def _queries(self, queries):
        if isinstance(queries, tuple) and len(queries) == 3:
            q_off, q_term, q_idf = (np.ascontiguousarray(a, t) for a, t in zip(queries, (np.uint32, np.uint32, np.float32)))
        else:
            q_off, q_term, q_idf = self.pack_queries([self.query_terms(q) if isinstance(q, str) else q for q in queries])
        return len(q_off) - 1, q_off, q_term, q_idf

    @property
    def slots(self):
        return int(N.lib().leann_bm25_slots(self._h))

    def __len__(self):
        return int(N.lib().leann_bm25_len(self._h))

    def _device_allow(self, allow):
        """an allow-bitmap for a *_device call: a numpy bitmap is uploaded (the returned DeviceArray keeps it alive for the call), a
        DeviceArray or a raw device pointer is passed through"""
        if isinstance(allow, DeviceArray):
            return allow.ptr, allow
        if isinstance(allow, np.ndarray):
            d = DeviceArray.from_host(np.ascontiguousarray(allow, np.uint8))
            return d.ptr, d
        return allow, None

    def search_batch(self, queries, top_k, allow=None, allow_stride=0):
        """Bm25Scorer::search per query.  queries: texts, lists of (term id, idf), or packed (q_off, q_term, q_idf).
        Returns pos [nq x top_k] u32, scores [nq x top_k] f32, counts [nq], n_positive [nq], min_max [nq x 2].
        allow: a bitmap over the passages (numpy u8, a DeviceArray or a device pointer; include/leann_backend.h "under an allow-bitmap"),
        query i's at byte i * allow_stride, stride 0 = one for the batch; None makes exactly the unfiltered call."""
        nq, q_off, q_term, q_idf = self._queries(queries)
        if allow is not None and not isinstance(allow, np.ndarray):  # already on the device: the device call, results downloaded
            return tuple(a.to_host() for a in self.search_batch_device((q_off, q_term, q_idf), top_k, allow=allow, allow_stride=allow_stride))
        pos = np.full((nq, top_k), 0xFFFFFFFF, np.uint32)
        sc = np.full((nq, top_k), -np.inf, np.float32)
        cnt, npos, mm = np.zeros(nq, np.uint32), np.zeros(nq, np.uint32), np.zeros((nq, 2), np.float32)
        q = (self._h, nq, _p(q_off, C.c_uint32), _p(q_term, C.c_uint32), _p(q_idf, C.c_float), top_k)
        o = (_p(pos, C.c_uint32), _p(sc, C.c_float), _p(cnt, C.c_uint32), _p(npos, C.c_uint32), _p(mm, C.c_float))
        if allow is None:
            N.check(N.lib().leann_bm25_search_batch(*q, *o))
        else:
            allow = np.ascontiguousarray(allow, np.uint8)
            need = (self.n_docs + 7) // 8 + (nq - 1) * allow_stride if allow_stride and nq else (self.n_docs + 7) // 8
            if allow.size < need:
                raise N.LeannError(1, f"Bm25Index.search_batch: the allow-bitmap holds {allow.size} bytes, {need} are needed")
            N.check(N.lib().leann_bm25_search_filtered_batch(*q, _p(allow, C.c_uint8), allow_stride, *o))
        return pos, sc, cnt, npos, mm

    def search_batch_device(self, queries, top_k, stream=None, out=None, allow=None, allow_stride=0):
        """search_batch with the results left in HBM: DeviceArrays (pos u32 [nq x top_k], scores f32, counts u32 [nq],
        n_positive u32 [nq], min_max f32 [nq x 2]); `out` reuses the arrays of an earlier call of the same shape."""
        nq, q_off, q_term, q_idf = self._queries(queries)
        if out is None:
            out = (DeviceArray((nq, top_k), np.uint32), DeviceArray((nq, top_k), np.float32), DeviceArray(nq, np.uint32),
                   DeviceArray(nq, np.uint32), DeviceArray((nq, 2), np.float32))
        q = (self._h, nq, _p(q_off, C.c_uint32), _p(q_term, C.c_uint32), _p(q_idf, C.c_float), top_k)
        o = (out[0].ptr, out[1].ptr, out[2].ptr, out[3].ptr, out[4].ptr, stream)
        if allow is None:
            N.check(N.lib().leann_bm25_search_batch_device(*q, *o))
        else:
            d_allow, keep = self._device_allow(allow)
            N.check(N.lib().leann_bm25_search_filtered_batch_device(*q, d_allow, allow_stride, *o))  # returns after the stream has finished
            del keep
        return out

    def hybrid_rerank_device(self, queries, d_keys, d_dists, d_counts, fetch_k, alpha, compat_polarity, top_k, stream=None, allow=None,
                             allow_stride=0):
        """The hybrid leg on lists in HBM (DeviceArrays or raw pointers: keys u64 / dists f32 [nq x fetch_k], counts u32 [nq]).
        Returns DeviceArrays (keys [nq x top_k] u64, scores f32, counts u32).  allow / allow_stride: as in search_batch."""
        nq, q_off, q_term, q_idf = self._queries(queries)
        ptr = lambda a: a.ptr if isinstance(a, DeviceArray) else a  # noqa: E731
        ok, os_, oc = DeviceArray((nq, top_k), np.uint64), DeviceArray((nq, top_k), np.float32), DeviceArray(nq, np.uint32)
        a = (self._h, nq, _p(q_off, C.c_uint32), _p(q_term, C.c_uint32), _p(q_idf, C.c_float), ptr(d_keys), ptr(d_dists), ptr(d_counts),
             fetch_k, alpha, 1 if compat_polarity else 0, top_k)
        o = (ok.ptr, os_.ptr, oc.ptr, stream)
        if allow is None:
            N.check(N.lib().leann_bm25_hybrid_rerank_device(*a, *o))
        else:
            d_allow, keep = self._device_allow(allow)
            N.check(N.lib().leann_bm25_hybrid_rerank_filtered_device(*a, d_allow, allow_stride, *o))
            del keep
        return ok, os_, oc

    def close(self):
        if getattr(self, "_h", None):
            N.lib().leann_bm25_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
