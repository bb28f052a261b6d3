"""Helper of the filtered-BM25 tests (not a test): the definition of the leann_bm25_*_filtered calls (include/leann_backend.h "under an
allow-bitmap") restated in numpy on top of tests/bm25_ref.py and oracle/searcher_oracle.py's hybrid_rerank.

Let A be the positions whose bit is set in a query's bitmap (bit i & 7 of byte i >> 3, bits at positions >= n_docs ignored).  The
score vector is Postings.score_query's, unchanged: idf, doc_len and avg_doc_len are the corpus's.  Everything after it sees that vector
restricted to A, with positions kept:
    search   the positives at positions in A through Postings.search (score descending, stable); n_positive their number; min_max
             folded over {scores[i] : i in A}
    hybrid   searcher.rs:146-169: bm25_top is that search at fetch_k, the ANN list enters as given, and hybrid_rerank folds min_b /
             max_b over {scores[i] : i in A} but looks a merged key up in the whole vector (scores[key], 0.0 beyond it)
    empty A  nothing comes back from either call; min_max is (+inf, -inf), the folds' identities

Also the masks and cases of tests/test_gpu_bm25_filtered.py, stated once so that tests/test_cpu_bm25_masked.py can hold each to the
branch it exists for without a device."""
import functools

import numpy as np

import bm25_ref
import hybrid_cases as hc
import searcher_oracle as so

f32 = np.float32
SIZES = (1, 7, 8, 9, 31, 32, 33, 255, 257, 8192, 8193, 16385)  # byte and word edges of the bitmap, boundaries of the sweep's ranges
KS = (1, 10, 1024)
MASKS = ("ones", "none", "last", "first", "alternating", "no_first_range", "no_best")


# ---- bitmaps ----------------------------------------------------------------------------------------------------------------------------
def nbytes(n_docs):
    return (n_docs + 7) // 8


def pack(member):
    """bool [n] -> bitmap u8 [ceil(n / 8)], pad bits zero"""
    return np.packbits(np.asarray(member, bool), bitorder="little")


def unpack(bitmap, n_docs):
    """bitmap -> bool [n_docs]; whatever the pad bits of the last byte hold is dropped"""
    return np.unpackbits(np.asarray(bitmap, np.uint8)[:nbytes(n_docs)], bitorder="little")[:n_docs].astype(bool)


def with_pad_bits(bitmap, n_docs):
    """the same bitmap with every bit at a position >= n_docs set"""
    out = np.array(bitmap, np.uint8)
    if n_docs % 8:
        out[nbytes(n_docs) - 1] |= np.uint8((0xFF << (n_docs % 8)) & 0xFF)
    return out


def strided(bitmaps, stride, fill=0xFF):
    """per-query bitmaps `stride` bytes apart; the bytes between them hold `fill`, which no query may read as its own"""
    out = np.full(stride * len(bitmaps), fill, np.uint8)
    for i, b in enumerate(bitmaps):
        assert len(b) <= stride
        out[i * stride:i * stride + len(b)] = b
    return out


def mask(name, n_docs, scores=None):
    """bool [n_docs] of a named mask; no_best needs the query's scores: the best passage (first of equals) is disallowed"""
    m = np.ones(n_docs, bool)
    if name == "ones":
        pass
    elif name == "none":
        m[:] = False
    elif name == "last":
        m[:] = False
        m[n_docs - 1] = True
    elif name == "first":
        m[:] = False
        m[0] = True
    elif name == "alternating":
        m[1::2] = False
    elif name == "no_first_range":
        m[:hc.CAP] = False  # the whole first row range of the sweep (all of a corpus that is no longer)
    elif name == "no_best":
        m[int(np.argmax(scores))] = False
    else:
        raise KeyError(name)
    return m


# ---- the definition ---------------------------------------------------------------------------------------------------------------------
class RestrictedScores:
    """what hybrid_rerank is handed as the BM25 score vector: iterating it (the min / max folds, bm25.rs:152-154) yields the scores
    at the allowed positions only, indexing it (bm25.rs:158) reads the whole vector"""

    def __init__(self, scores, member):
        self.scores, self.member = scores, member

    def __iter__(self):
        return iter(self.scores[self.member])

    def __len__(self):
        return len(self.scores)

    def __getitem__(self, i):
        return self.scores[i]


def restrict(scores, member):
    """the score vector as the selection sees it: positions kept, a disallowed position can never be a positive"""
    return np.where(member, scores, f32(0.0)).astype(np.float32)


def search(post, terms, top_k, member, scores=None):
    """(positions u32, scores f32, n_positive, (min, max)) of the masked search"""
    s = post.score_query(terms) if scores is None else scores
    pos, sc = post.search(terms, top_k, scores=restrict(s, member))
    inside = s[member]
    mm = (f32(np.inf), f32(-np.inf)) if not member.any() else (inside.min(), inside.max())
    return pos, sc, int((inside > 0).sum()), mm


def hybrid(post, terms, keys, dists, member, alpha, compat, fetch_k, top_k, scores=None):
    """[(key, f32 score)] of the masked hybrid leg, best first, cut to top_k"""
    if not member.any():
        return []
    s = post.score_query(terms) if scores is None else scores
    top = post.search(terms, fetch_k, scores=restrict(s, member))[0]
    vr = [(int(k), f32(d) if compat else f32(f32(1.0) - f32(d))) for k, d in zip(keys, dists)]
    have = {i for i, _ in vr}
    for p in top:
        if int(p) not in have:
            vr.append((int(p), f32(0.0)))
    return so.hybrid_rerank(vr, RestrictedScores(s, member), alpha)[:top_k]


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
def tie_mask(n_docs):
    """boundary_corpus plants equal scores on its last two rows (query [tie]): the earlier one — the winner of the tie — is disallowed"""
    m = np.ones(n_docs, bool)
    m[n_docs - 2] = False
    return m


RISING_N = 24577


@functools.lru_cache(maxsize=None)
def rising_mask(q):
    """masks over rising_corpus(RISING_N) that keep the overflow: the sweep's third range, rows [16384, 24577), brings 8193 rows of
    rising scores; disallowing rows only below 16384 leaves all of them survivors.  Query-dependent so that a stride is exercised:
    q % 3 == 0 every 2nd early row, 1 every 3rd, 2 the first 5000 rows."""
    m = np.ones(RISING_N, bool)
    if q % 3 == 0:
        m[0:16384:2] = False
    elif q % 3 == 1:
        m[1:16384:3] = False
    else:
        m[:5000] = False
    m.setflags(write=False)
    return m


LARGE_CASE = "large_m_256"  # hybrid_cases: fetch_k = 256, top_k up to 512, 40 queries over the small corpus
LARGE_INJECTED_OUT = 10     # query 4 (empty ANN list: all of bm25_top is injected) loses the first 10 entries of its bm25_top


@functools.lru_cache(maxsize=None)
def large_masks():
    """per query of LARGE_CASE: even queries lose their best BM25 passage (max_b moves: other score bits than the unmasked call's),
    query 4 loses the head of its bm25_top, query 5 (no known token, a full ANN list) is allowed nothing; odd queries keep everything"""
    c = hc.case(LARGE_CASE)
    post = hc.post_of(c)
    out = []
    for q, terms in enumerate(c["queries"]):
        m = np.ones(post.n_docs, bool)
        pos = hc.positives(c, q)
        if q % 2 == 0 and pos:
            m[pos[0][0]] = False
        if q == 4:
            m[[p for p, _ in pos[:LARGE_INJECTED_OUT]]] = False
        if q == 5:
            m[:] = False
        m.setflags(write=False)
        out.append(m)
    return out


STRIDE_CASE = dict(corpus="chunked", nq=2 * hc.SLOTS + 5, stride=nbytes(3001) + 3)  # 379 bytes: not a multiple of 4


@functools.lru_cache(maxsize=None)
def stride_masks():
    """one bitmap per query of hybrid_cases' chunked case: a third of the passages allowed at random, some queries all or nothing"""
    rng = np.random.default_rng(77)
    n = hc.corpus("chunked").n_docs
    out = []
    for q in range(STRIDE_CASE["nq"]):
        m = rng.random(n) < (0.05, 0.33, 0.9)[q % 3]
        if q in (5, 64, 132):
            m[:] = False
        if q in (6, 65):
            m[:] = True
        m.setflags(write=False)
        out.append(m)
    return out
