"""The inputs of tests/test_gpu_hybrid_edges.py, stated once so that tests/test_cpu_hybrid_cases.py can hold every case to the branch it
exists for without a device (the pattern of tests/delete_cases.py and build_ref.CASES).

Three kinds of things live here:
  * sweep_ranges / sweep_survivors: the host loop of bm25_run and the survivor test of bm25_emit_kernel (csrc/bm25.hip) in numpy — which
    rows a launch sweeps and how many of them are appended to a query's candidate list.  A list overflows when a launch appends more
    than `cap` keys (fold_candidates_kernel tests m > cap); the overflow cannot be seen through the ABI, so the CPU suite shows on
    these restatements that a corpus takes that path.
  * corpora: rising_corpus (scores strictly rising with the position: every row of every range survives) and boundary_corpus (a
    corpus that ends on, or one row past, a range boundary, with the best passage at the last position and a tie on the last two rows).
  * rerank cases: (keys, dists, counts) lists plus query terms over a small Zipf corpus, with fetch_k, stride and top_k stated, and the
    expected answers from oracle/searcher_oracle.py (the sparse forms) on tests/bm25_ref.py scores.

Everything is seeded; corpus(), case() and positives() are computed once per process and must not be modified by their callers."""
import functools

import numpy as np

import bm25_ref
import searcher_oracle as so

f32 = np.float32
U64MAX = np.iinfo(np.uint64).max
CAP = 8192         # BM25_CAND_CAP: entries of a candidate list, and the length of the first row range
SLOTS = 64         # BM25_MAX_SLOTS: queries per chunk for any corpus below 4.19 M passages
MAX_FETCH = 256    # HYB_MAX_FETCH
MAX_MERGED = 512   # HYB_MAX_MERGED
ALPHAS = (0.0, 0.7, 1.0)
RISING_KS = (1, 10, 256, 1024)
BOUNDARY_SIZES = (1, 2, 255, 257, 8192, 8193, 16384, 16385)


# ---- the selection sweep ----------------------------------------------------------------------------------------------------------------
def orderable(scores):
    """f32_orderable of common.cuh: u32 whose unsigned order is the floats' order"""
    u = np.ascontiguousarray(scores, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def selection_keys(scores, rows):
    """~orderable(score) << 32 | row: ascending = score descending, position ascending"""
    return ((~orderable(scores)).astype(np.uint64) << np.uint64(32)) | np.asarray(rows, np.uint64)


def sweep_ranges(n_docs, first=CAP):
    """the [r0, r1) of every bm25_emit_kernel launch: `first` rows, then each range as long as all rows seen so far"""
    out, r0, length = [], 0, first
    while r0 < n_docs:
        r1 = min(r0 + length, n_docs)
        out.append((r0, r1))
        r0 = r1
        length = r0
    return out


def sweep_survivors(scores, k, cap=CAP):
    """Keys appended per range: a positive row survives when its key is below the running k-th best key (all ones while fewer than k
    are known), which is fixed for a launch and refolded after it.  The counts are those of a sweep in which no list has overflowed
    yet: from the first count above `cap` on the device drops keys and the chunk is selected again by the segment sorter."""
    best = np.full(k, U64MAX, np.uint64)
    counts = []
    for r0, r1 in sweep_ranges(len(scores)):
        s = scores[r0:r1]
        rows = np.arange(r0, r1, dtype=np.uint64)
        keys = selection_keys(s[s > 0], rows[s > 0])
        keys = keys[keys < best[k - 1]]
        counts.append(len(keys))
        best = np.sort(np.concatenate([best, keys]))[:k]
    return counts


def overflows(counts, cap=CAP):
    return any(c > cap for c in counts)


# ---- corpora ----------------------------------------------------------------------------------------------------------------------------
RISING_QUERIES = ([0], [1], [0, 1], [], [0, 0])


@functools.lru_cache(maxsize=None)
def rising_corpus(n):
    """term 0 on every passage with tf = 1 and doc_len[i] = n - i: the score of a passage rises strictly with its position, and every
    passage is positive.  Term 1 on passages 5, 6, 7, as in test_rising_scores_overflow_the_candidate_lists, for two-token queries."""
    post_off = np.array([0, n, n + 3], np.uint64)
    post_doc = np.concatenate([np.arange(n), [5, 6, 7]]).astype(np.uint32)
    post_tf = np.ones(n + 3, np.uint32)
    doc_len = (n - np.arange(n)).astype(np.uint32)
    return bm25_ref.Postings(n, post_off, post_doc, post_tf, doc_len, f32(n + 1) / f32(2.0))


def _with_terms(post, extra, doc_len):
    """post with further terms appended to its vocabulary — extra = [[(passage, tf), ...] ascending, ...] — and other passage lengths"""
    off = [int(x) for x in post.post_off]
    for lst in extra:
        off.append(off[-1] + len(lst))
    doc = np.concatenate([post.post_doc, [p for lst in extra for p, _ in lst]]).astype(np.uint32)
    tf = np.concatenate([post.post_tf, [t for lst in extra for _, t in lst]]).astype(np.uint32)
    return bm25_ref.Postings(post.n_docs, np.array(off, np.uint64), doc, tf, doc_len, post.avg_doc_len)


BOUNDARY_TERMS = 50


@functools.lru_cache(maxsize=None)
def boundary_corpus(n):
    """n passages of 2 to 6 tokens over BOUNDARY_TERMS Zipf terms (n <= 2: hand-written) plus two planted terms:
    `best`: on the last passage alone, tf = 3 — any query with it has its best passage at position n - 1;
    `tie`:  on the last two passages, tf = 1, equal lengths — equal f32 scores on rows n - 2 and n - 1, which for n = 8193 and 16385
            lie on either side of a range boundary and for n = 257 on either side of a workgroup's 256 rows.
    Returns (Postings, best term, tie term, queries): 1 to 3 tokens with repeats, and one empty query."""
    if n == 1:    # term 0 on the passage, term 1 on none (an empty list), best = 2, tie = 3 (one row: no tie)
        post = bm25_ref.Postings(1, np.array([0, 1, 1, 2, 3], np.uint64), np.array([0, 0, 0], np.uint32), np.array([2, 3, 1], np.uint32),
                                 np.array([3], np.uint32), 3.0)
        return post, 2, 3, ([0], [1], [2], [3], [3, 3], [0, 2, 0], [1, 0], [])
    if n == 2:    # term 0 on both with equal lengths: a tie over the whole corpus; term 1 on none
        post = bm25_ref.Postings(2, np.array([0, 2, 2, 3, 5], np.uint64), np.array([0, 1, 1, 0, 1], np.uint32),
                                 np.array([1, 1, 3, 1, 1], np.uint32), np.array([4, 4], np.uint32), 4.0)
        return post, 2, 3, ([0], [1], [2], [3], [3, 3], [0, 2, 0], [1, 0], [])
    base = bm25_ref.synth_corpus(7000 + n, n, BOUNDARY_TERMS, len_lo=2, len_hi=6)
    doc_len = base.doc_len.copy()
    doc_len[n - 2] = doc_len[n - 1]
    best, tie = BOUNDARY_TERMS, BOUNDARY_TERMS + 1
    post = _with_terms(base, [[(n - 1, 3)], [(n - 2, 1), (n - 1, 1)]], doc_len)
    return post, best, tie, ([best], [tie], [tie, tie], [0, best, 0], [1, 2], [0], [3, tie, 1], [])


def term_ids_by_df(post, lo, hi):
    df = np.diff(post.post_off.astype(np.int64))
    return [int(t) for t in np.flatnonzero((df >= lo) & (df <= hi))]


@functools.lru_cache(maxsize=None)
def corpus(name):
    if name == "small":    # cases (a), (b): short passages, few distinct (tf, length) pairs: large groups of equal scores
        return bm25_ref.synth_corpus(41, 5003, 400, len_lo=3, len_hi=9)
    if name == "chunked":  # case (c)
        return bm25_ref.synth_corpus(43, 3001, 600, len_lo=5, len_hi=15)
    if name == "stream":   # case (f): as many passages as the graph handle has rows
        return bm25_ref.synth_corpus(47, 4000, 500, len_lo=5, len_hi=15)
    if name.startswith("rising_"):
        return rising_corpus(int(name[7:]))
    raise KeyError(name)


def random_queries(rng, post, nq, df_lo, df_hi, max_tokens=3):
    terms = term_ids_by_df(post, df_lo, df_hi)
    out = []
    for _ in range(nq):
        q = [int(t) for t in rng.choice(terms, size=int(rng.integers(1, max_tokens + 1)))]
        if len(q) > 1 and rng.random() < 0.3:
            q[-1] = q[0]  # a repeated token counts twice (bm25.rs:81)
        out.append(q)
    return out


# ---- rerank cases -----------------------------------------------------------------------------------------------------------------------
def _dists(rng, c):
    d = np.sort(rng.uniform(0.02, 1.3, size=c)).astype(np.float32)
    if c > 4:
        d[1:4] = d[1]  # equal distances
    return d


def _list(rng, n_docs, count, must=(), avoid=()):
    """`count` distinct positions: those of `must`, filled up with others outside `avoid`, in random order"""
    chosen = list(dict.fromkeys(int(x) for x in must))[:count]
    taken = set(chosen) | {int(x) for x in avoid}
    while len(chosen) < count:
        x = int(rng.integers(0, n_docs))
        if x not in taken:
            taken.add(x)
            chosen.append(x)
    return [chosen[i] for i in rng.permutation(len(chosen))]


def _blank(nq, fetch_k):
    return np.full((nq, fetch_k), U64MAX, np.uint64), np.full((nq, fetch_k), np.inf, np.float32), np.zeros(nq, np.uint32)


def _put(keys, dists, counts, q, lst, d):
    keys[q, :len(lst)], dists[q, :len(lst)], counts[q] = lst, d, len(lst)


def _top(post, terms, fetch_k):
    return [int(p) for p in post.search(terms, fetch_k)[0]]


def _large_m(fetch_k):
    """40 queries over the small corpus whose merged lists reach 2 * fetch_k.  With `top` = the query's bm25_top (fetch_k entries):
         0  no ANN key in top                      m = 2 fetch_k                    (512 at fetch_k = 256)
         1  a third of top among the ANN keys      fetch_k < m < 2 fetch_k          + the planted tie, see below
         2  all of top but one                     m = fetch_k + 1
         3  the ANN list is top                    m = fetch_k
         4  empty ANN list                         m = fetch_k, all injected
         5  no known token, full ANN list          m = fetch_k, nothing injected
         6  no known token, empty ANN list         m = 0
         7  a rare term, half an ANN list
         8+ random: 1 to 3 tokens, ANN lists of any length, up to a third of them from top
    Query 1's tie: A, B, C are three entries of top with the same BM25 score; A and B are ANN keys at distances 0.0 and 1.0, C is not
    an ANN key.  C is injected with vector score 0.0, which is A's under the reference's polarity and B's under the corrected one, so
    C's blended score equals A's or B's at every alpha: a tie between a list position below fetch_k and one at or above it."""
    post = corpus("small")
    rng = np.random.default_rng(9000 + fetch_k)
    nq = 40
    frequent = min(term_ids_by_df(post, 300, 900), key=post.df)
    rare = min(term_ids_by_df(post, 5, 60), key=post.df)
    queries = [[frequent], [frequent], [frequent], [frequent], [frequent], [], [], [rare]] + random_queries(rng, post, nq - 8, 20, 1200)
    keys, dists, counts = _blank(nq, fetch_k)
    top = _top(post, [frequent], fetch_k)
    assert len(top) == fetch_k
    _put(keys, dists, counts, 0, _list(rng, post.n_docs, fetch_k, avoid=top), _dists(rng, fetch_k))
    # query 1
    sc = post.score_query([frequent])[top].view(np.uint32)
    vals, cnt = np.unique(sc, return_counts=True)
    group = [top[i] for i in np.flatnonzero(sc == vals[np.argmax(cnt)])]
    assert len(group) >= 3
    a, b, c = group[0], group[1], group[-1]
    must = [a, b] + [p for p in top[::3] if p not in (a, b, c)]
    lst = _list(rng, post.n_docs, fetch_k, must=must, avoid=top)
    d = _dists(rng, fetch_k)
    lst.remove(a), lst.remove(b)
    lst = [a] + lst
    at = int(np.searchsorted(d, 1.0))
    lst.insert(at, b)
    d[0], d[at] = 0.0, 1.0
    _put(keys, dists, counts, 1, lst, d)
    _put(keys, dists, counts, 2, _list(rng, post.n_docs, fetch_k, must=top[:fetch_k - 1], avoid=top), _dists(rng, fetch_k))
    _put(keys, dists, counts, 3, _list(rng, post.n_docs, fetch_k, must=top), _dists(rng, fetch_k))
    _put(keys, dists, counts, 5, _list(rng, post.n_docs, fetch_k), _dists(rng, fetch_k))
    _put(keys, dists, counts, 7, _list(rng, post.n_docs, fetch_k // 2, must=_top(post, [rare], 2)), _dists(rng, fetch_k // 2))
    for q in range(8, nq):
        c_ = fetch_k if q % 3 else int(rng.integers(0, fetch_k + 1))
        t = _top(post, queries[q], fetch_k)
        must = [t[i] for i in rng.permutation(len(t))[:int(rng.integers(0, c_ // 3 + 1))]]
        _put(keys, dists, counts, q, _list(rng, post.n_docs, c_, must=must), _dists(rng, c_))
    return dict(corpus="small", fetch_k=fetch_k, stride=MAX_FETCH, top_ks=(1, 51, 257, 512), queries=queries, keys=keys, dists=dists,
                counts=counts, tie=dict(query=1, a=a, b=b, c=c))


def _clamps():
    """Arguments the code clamps or widens, fetch_k = 40, stride = 64:
         0  counts = fetch_k + 9: the arrays hold fetch_k entries a row, the first fetch_k count
         1  keys n_docs + 5 (beyond the score vector: BM25 score 0.0) and 2^40 + p, p = the query's best BM25 position, which is not
            otherwise in the list: a 32-bit compare would take the wide key for p and suppress p's injection
         2  the sparse call is told stride + 17 positives and handed `stride` of them: P = min(count, stride)
         3  counts = fetch_k + 9 again, on a query of other terms
         4..6 plain queries; the last row claims nothing it does not hold, so a missing clamp misreads a neighbour's row, not past the end"""
    post = corpus("small")
    rng = np.random.default_rng(9500)
    fetch_k, stride, nq = 40, 64, 7
    big = min(term_ids_by_df(post, stride + 17, 400), key=post.df)  # at least stride + 17 positives
    queries = [[big], [big], [big], random_queries(rng, post, 1, 20, 400)[0]] + random_queries(rng, post, 3, 20, 400)
    keys, dists, counts = _blank(nq, fetch_k)
    for q in range(nq):
        t = _top(post, queries[q], fetch_k)
        _put(keys, dists, counts, q, _list(rng, post.n_docs, fetch_k, must=t[3:12]), _dists(rng, fetch_k))
    p = _top(post, [big], 1)[0]
    lst = _list(rng, post.n_docs, fetch_k - 2, avoid=[p])
    lst.insert(3, post.n_docs + 5)
    lst.insert(17, 2 ** 40 + p)
    keys[1] = lst
    counts[0] = counts[3] = fetch_k + 9
    return dict(corpus="small", fetch_k=fetch_k, stride=stride, top_ks=(10,), queries=queries, keys=keys, dists=dists, counts=counts,
                sparse_claim={2: stride + 17}, wide=dict(query=1, p=p, key=2 ** 40 + p))


def _ones():
    """fetch_k = top_k = 1: m = 0, 1 or 2
         0  no ANN key, no token           m = 0
         1  no ANN key, positives          m = 1, injected
         2  the ANN key is the best BM25 position   m = 1
         3  the ANN key is another position         m = 2, one of them returned
         4  an ANN key, no token           m = 1
         5  an ANN key beyond the score vector, positives   m = 2"""
    post = corpus("small")
    t = term_ids_by_df(post, 20, 400)[0]
    p = _top(post, [t], 1)[0]
    queries = [[], [t], [t], [t], [], [t]]
    keys, dists, counts = _blank(6, 1)
    for q, key in ((2, p), (3, (p + 1) % post.n_docs), (4, 77), (5, post.n_docs + 5)):
        keys[q, 0], dists[q, 0], counts[q] = key, 0.4, 1
    return dict(corpus="small", fetch_k=1, stride=4, top_ks=(1,), queries=queries, keys=keys, dists=dists, counts=counts)


def _chunked():
    """2 * 64 + 5 queries: three chunks of the dense call, the last of 5.  Queries 70 and 131 have no known token, 66 and 100 an empty
    ANN list, 130 a short one: all in a chunk other than the first, where every per-query pointer carries its q0 offset."""
    post = corpus("chunked")
    rng = np.random.default_rng(9700)
    fetch_k, nq = 50, 2 * SLOTS + 5
    queries = random_queries(rng, post, nq, 3, 400, max_tokens=4)
    queries[70], queries[131] = [], []
    keys, dists, counts = _blank(nq, fetch_k)
    for q in range(nq):
        c = 0 if q in (66, 100) else 7 if q == 130 else fetch_k if q % 5 else int(rng.integers(1, fetch_k))
        t = _top(post, queries[q], fetch_k)
        must = [t[i] for i in rng.permutation(len(t))[:c // 3]]
        _put(keys, dists, counts, q, _list(rng, post.n_docs, c, must=must), _dists(rng, c))
    return dict(corpus="chunked", fetch_k=fetch_k, stride=MAX_FETCH, top_ks=(10,), queries=queries, keys=keys, dists=dists, counts=counts)


def _rising_hybrid():
    """The dense call on the rising corpus of 24 577 passages, fetch_k = 256: queries 0, 2, 4, 5 overflow their lists (all rows of the
    third range survive), 1 (three positives) and 3 (no token) do not, and all share a chunk, which the segment sorter reselects as a
    whole: bm25_top is then read from the keys bm25_rebuild_best_kernel wrote.  The ANN lists mix the first positions (lowest scores)
    with the last ones (the highest: members of bm25_top)."""
    n = 24577
    rng = np.random.default_rng(9900)
    fetch_k = MAX_FETCH
    queries = [[0], [1], [0, 1], [], [0, 0], [0]]
    keys, dists, counts = _blank(len(queries), fetch_k)
    early, late = np.arange(0, 400), np.arange(n - 400, n)
    for q, c in enumerate((256, 256, 200, 256, 131, 0)):
        lst = [int(x) for x in rng.permutation(np.concatenate([rng.choice(early, c // 2, replace=False),
                                                               rng.choice(late, c - c // 2, replace=False)]))]
        _put(keys, dists, counts, q, lst, _dists(rng, c))
    return dict(corpus=f"rising_{n}", fetch_k=fetch_k, stride=MAX_FETCH, top_ks=(20,), queries=queries, keys=keys, dists=dists, counts=counts)


_MAKERS = {"large_m_128": lambda: _large_m(128), "large_m_255": lambda: _large_m(255), "large_m_256": lambda: _large_m(256),
           "clamps": _clamps, "ones": _ones, "chunked": _chunked, "rising_hybrid": _rising_hybrid}
CASES = tuple(_MAKERS)


@functools.lru_cache(maxsize=None)
def case(name):
    c = _MAKERS[name]()
    c["name"] = name
    for a in (c["keys"], c["dists"], c["counts"]):
        a.setflags(write=False)
    return c


def post_of(c):
    return corpus(c["corpus"])


@functools.lru_cache(maxsize=None)
def _positives(corpus_name, terms):
    pos, sc = corpus(corpus_name).search(list(terms), corpus(corpus_name).n_docs)
    return [(int(p), f32(s)) for p, s in zip(pos, sc)]


def positives(c, q):
    """all positives of query q, [(position, f32 score)], sorted as Bm25Scorer::search sorts them"""
    return _positives(c["corpus"], tuple(c["queries"][q]))


def n_list(c, q):
    """entries of query q's ANN list that count: min(counts[q], fetch_k)"""
    return min(int(c["counts"][q]), c["fetch_k"])


def n_sparse(c, q):
    """positives the sparse call works with: min(count, stride)"""
    return min(len(positives(c, q)), c["stride"])


def merged_len(c, q, sparse=False):
    """m: the ANN entries plus the entries of bm25_top that are not among them"""
    n = n_list(c, q)
    have = {int(k) for k in c["keys"][q, :n]}
    pos = positives(c, q)[:n_sparse(c, q)] if sparse else positives(c, q)
    return n + sum(1 for p, _ in pos[:c["fetch_k"]] if p not in have)


def sparse_arrays(c):
    """(pos u32, score f32) [nq x stride] and count [nq] of the sparse call: the first `stride` positives; count = min(P, stride)
    unless the case claims more for a query (sparse_claim)"""
    nq, stride = len(c["queries"]), c["stride"]
    pos = np.full((nq, stride), 0xFFFFFFFF, np.uint32)
    sc = np.zeros((nq, stride), np.float32)
    cnt = np.zeros(nq, np.uint32)
    for q in range(nq):
        p = positives(c, q)[:stride]
        pos[q, :len(p)], sc[q, :len(p)], cnt[q] = [x for x, _ in p], [x for _, x in p], len(p)
    for q, claim in c.get("sparse_claim", {}).items():
        assert len(positives(c, q)) >= claim and cnt[q] == stride
        cnt[q] = claim
    return pos, sc, cnt


def expected(c, q, alpha, compat, sparse=False, top_k=MAX_MERGED):
    """searcher_oracle.hybrid_leg_sparse on the entries that count; sparse: with the first min(count, stride) positives only — the BM25
    side the sparse call is defined on (include/leann_backend.h) — else with all of them: the dense call"""
    n = n_list(c, q)
    pos = positives(c, q)[:n_sparse(c, q)] if sparse else positives(c, q)
    return so.hybrid_leg_sparse(c["keys"][q, :n], c["dists"][q, :n], pos, post_of(c).n_docs, alpha, top_k, c["fetch_k"], compat)


def position_scores(c, q, alpha, compat):
    """the blended f32 score of every position of query q's merged list (dense call), in list order"""
    n = n_list(c, q)
    merged = [int(k) for k in c["keys"][q, :n]]
    have = set(merged)
    merged += [p for p, _ in positives(c, q)[:c["fetch_k"]] if p not in have]
    by_key = dict(expected(c, q, alpha, compat))
    assert len(by_key) == len(merged)
    return np.array([by_key[k] for k in merged], np.float32)


def packed(post, queries):
    q_off = np.zeros(len(queries) + 1, np.uint32)
    q_off[1:] = np.cumsum([len(q) for q in queries])
    q_term = np.array([t for q in queries for t in q], np.uint32)
    q_idf = np.array([post.idf(t) for q in queries for t in q], np.float32)
    return q_off, q_term, q_idf
