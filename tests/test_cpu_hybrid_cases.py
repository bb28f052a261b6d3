"""CPU suite: every case of tests/hybrid_cases.py reaches the branch of csrc/hybrid_rerank.cuh / csrc/bm25.hip it exists for, shown on
the references alone (oracle/searcher_oracle.py, tests/bm25_ref.py and the numpy restatement of the selection sweep).  No GPU and no
library: tests/test_gpu_hybrid_edges.py then holds the device to the same cases."""
import numpy as np
import pytest

import hybrid_cases as hc


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


# ---- merged lists above 256 entries -----------------------------------------------------------------------------------------------------
def test_large_m_cases_reach_the_second_stride_of_every_loop():
    c = hc.case("large_m_256")
    assert c["fetch_k"] == hc.MAX_FETCH and max(c["top_ks"]) == hc.MAX_MERGED
    m = [hc.merged_len(c, q) for q in range(len(c["queries"]))]
    assert m[0] == 512 and hc.n_list(c, 0) == 256  # 256 ANN keys, 256 injected: s_inj full, the 512-wide sort
    assert 256 < m[1] < 512
    assert m[2] == 257
    assert m[3] == 256 and m[4] == 256 and hc.n_list(c, 4) == 0
    assert m[6] == 0
    assert any(x < hc.MAX_MERGED for x in m)        # top_k = 512 exceeds m: the tail fill
    assert sum(x > 256 for x in m) >= 10
    # the sparse call sees the same lists where the positives fit the stride, and reaches 512 as well
    ms = [hc.merged_len(c, q, sparse=True) for q in range(len(c["queries"]))]
    assert ms[0] == 512 and ms[2] == 257
    assert any(len(hc.positives(c, q)) > c["stride"] for q in range(len(m)))        # P = min(count, stride) cuts something ...
    assert sum(0 < len(hc.positives(c, q)) <= c["stride"] for q in range(len(m))) >= 5  # ... and the two calls can be compared
    for name, least in (("large_m_255", 510), ("large_m_128", 256)):
        o = hc.case(name)
        assert hc.merged_len(o, 0) == least and hc.merged_len(o, 2) == o["fetch_k"] + 1


@pytest.mark.parametrize("name", ["large_m_128", "large_m_255", "large_m_256"])
@pytest.mark.parametrize("compat", [True, False])
def test_large_m_cases_tie_across_the_end_of_the_ann_list(name, compat):
    """query 1: an injected entry (position >= fetch_k) has the blended f32 score of an ANN entry (position < fetch_k), at every alpha"""
    c = hc.case(name)
    t, F = c["tie"], c["fetch_k"]
    keys = [int(k) for k in c["keys"][t["query"], :F]]
    assert t["c"] not in keys and keys.index(t["a"]) < F and keys.index(t["b"]) < F
    for alpha in hc.ALPHAS:
        s = _bits(hc.position_scores(c, t["query"], alpha, compat))
        assert F < len(s) < 2 * F
        low, high = set(s[:F].tolist()), set(s[F:].tolist())
        assert low & high, (name, alpha, compat)
        if F == hc.MAX_FETCH:
            assert set(s[:256].tolist()) & set(s[256:].tolist())  # across the 256-thread stride of the body's loops
        exp = hc.expected(c, t["query"], alpha, compat)
        ids = [i for i, _ in exp]
        partner = t["a"] if compat else t["b"]
        assert ids.index(partner) < ids.index(t["c"])          # the stable order: the earlier list position first
        assert _bits(dict(exp)[partner]) == _bits(dict(exp)[t["c"]])


# ---- the rising corpus ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,last", [(24576, 8192), (24577, 8193)])
def test_rising_corpus_fills_its_lists_exactly_or_by_one_more(n, last):
    post = hc.rising_corpus(n)
    s = post.score_query([0])
    assert s.dtype == np.float32 and (s > 0).all() and (np.diff(s.astype(np.float64)) > 0).all()  # strictly rising f32 values
    assert hc.sweep_ranges(n) == [(0, 8192), (8192, 16384), (16384, n)]
    for k in hc.RISING_KS:
        counts = hc.sweep_survivors(s, k)
        assert counts == [8192, 8192, last], (n, k)
        assert hc.overflows(counts) == (last > hc.CAP)
    for terms in hc.RISING_QUERIES:  # what the other queries of the GPU test do
        sq = post.score_query(terms)
        for k in hc.RISING_KS:
            counts = hc.sweep_survivors(sq, k)
            if terms in ([0], [0, 0]):
                assert max(counts) == last
            elif 0 not in terms:
                assert max(counts) <= 3 and not hc.overflows(counts)


def test_rising_hybrid_case_mixes_overflowing_and_quiet_slots_in_one_chunk():
    c = hc.case("rising_hybrid")
    post = hc.post_of(c)
    assert post.n_docs == 24577 and len(c["queries"]) <= hc.SLOTS and c["fetch_k"] == hc.MAX_FETCH
    over = [hc.overflows(hc.sweep_survivors(post.score_query(t), c["fetch_k"])) for t in c["queries"]]
    assert over == [True, False, True, False, True, True]
    assert c["queries"][3] == []
    n = post.n_docs
    for q in (0, 2, 4):  # early (low scores) and late positions in one list, some of the late ones members of bm25_top
        keys = c["keys"][q, :hc.n_list(c, q)].astype(np.int64)
        top = {p for p, _ in hc.positives(c, q)[:c["fetch_k"]]}
        assert (keys < 400).any() and (keys >= n - 400).any()
        assert 0 < len(top & set(keys.tolist())) < len(top)
    assert hc.merged_len(c, 5) == 256 and hc.n_list(c, 5) == 0


# ---- corpora at the sweep's range boundaries --------------------------------------------------------------------------------------------
def test_sweep_ranges_at_and_past_a_boundary():
    assert hc.sweep_ranges(8192) == [(0, 8192)]
    assert hc.sweep_ranges(8193) == [(0, 8192), (8192, 8193)]
    assert hc.sweep_ranges(16384) == [(0, 8192), (8192, 16384)]
    assert hc.sweep_ranges(16385) == [(0, 8192), (8192, 16384), (16384, 16385)]
    assert hc.sweep_ranges(1) == [(0, 1)] and hc.sweep_ranges(257) == [(0, 257)]
    assert hc.sweep_ranges(200_000)[-1] == (131072, 200_000)  # 8192, 8192, 16384, ...: each range as long as all rows before it
    for n in hc.BOUNDARY_SIZES:
        r = hc.sweep_ranges(n)
        assert r[0][0] == 0 and r[-1][1] == n and all(a[1] == b[0] for a, b in zip(r, r[1:]))


@pytest.mark.parametrize("n", hc.BOUNDARY_SIZES)
def test_boundary_corpora_plant_the_best_passage_last_and_a_tie_on_the_last_rows(n):
    post, best, tie, queries = hc.boundary_corpus(n)
    assert post.n_docs == n and [] in queries and any(len(q) == 3 and len(set(q)) < 3 for q in queries)
    assert {len(q) for q in queries} >= {0, 1, 2, 3}
    for terms in queries:
        if best in terms:
            s = post.score_query(terms)
            assert int(post.search(terms, 1, scores=s)[0][0]) == n - 1 and (s[:n - 1] < s[n - 1]).all()
    s = post.score_query([tie])
    if n >= 2:
        assert _bits(s[n - 2]) == _bits(s[n - 1]) and s[n - 1] > 0 and int((s > 0).sum()) == 2
        assert int(post.search([tie], 1, scores=s)[0][0]) == n - 2  # the tie of the k-th score at k = 1: the earlier position wins
        if n in (8193, 16385):
            assert hc.sweep_ranges(n)[-1] == (n - 1, n)             # ... and the two rows are swept by different launches
    if n >= 255:
        assert int((post.score_query([0]) > 0).sum()) > 64          # top_k = 1 cuts, top_k = 1024 > n_docs does not (n < 1024)


# ---- clamps, widening, fetch_k = 1 ------------------------------------------------------------------------------------------------------
def test_clamp_case_holds_what_it_claims():
    import searcher_oracle as so
    c = hc.case("clamps")
    F, n_docs = c["fetch_k"], hc.post_of(c).n_docs
    assert c["counts"][0] == F + 9 and c["counts"][3] == F + 9 and c["keys"].shape[1] == F and c["counts"][-1] <= F
    w = c["wide"]
    keys = [int(k) for k in c["keys"][w["query"]]]
    assert w["key"] in keys and w["key"] >> 32 != 0 and (w["key"] & 0xFFFFFFFF) == w["p"]
    assert w["p"] not in keys and w["p"] == hc.positives(c, w["query"])[0][0] and n_docs + 5 in keys
    for sparse in (False, True):
        exp = dict(hc.expected(c, w["query"], 0.7, True, sparse=sparse))
        assert w["key"] in exp and w["p"] in exp  # the wide key stays, and the position it aliases is injected all the same
        assert len(exp) == hc.merged_len(c, w["query"], sparse=sparse)
    pos, sc, cnt = hc.sparse_arrays(c)
    assert cnt[2] == c["stride"] + 17 and pos.shape[1] == c["stride"] and hc.n_sparse(c, 2) == c["stride"]
    # cutting at the stride changes the answer's scores: min(count, stride) is not a formality
    cut, whole = hc.expected(c, 2, 0.7, True, sparse=True), hc.expected(c, 2, 0.7, True)
    assert len(hc.positives(c, 2)) >= c["stride"] + 17 and cut != whole
    # hybrid_leg_sparse is the dense restatement on these inputs
    dense = np.zeros(n_docs, np.float32)
    for p, s in hc.positives(c, 4):
        dense[p] = s
    n = hc.n_list(c, 4)
    vr = [(int(k), np.float32(d)) for k, d in zip(c["keys"][4, :n], c["dists"][4, :n])]
    have = {i for i, _ in vr}
    vr += [(p, np.float32(0.0)) for p, _ in hc.positives(c, 4)[:F] if p not in have]
    a, b = so.hybrid_rerank(vr, dense, 0.7), hc.expected(c, 4, 0.7, True)
    assert [i for i, _ in a] == [i for i, _ in b] and (_bits([s for _, s in a]) == _bits([s for _, s in b])).all()


def test_ones_case_has_every_merged_length():
    c = hc.case("ones")
    assert c["fetch_k"] == 1 and c["top_ks"] == (1,)
    assert [hc.merged_len(c, q) for q in range(6)] == [0, 1, 1, 2, 1, 2]


# ---- more queries than slots ------------------------------------------------------------------------------------------------------------
def test_chunked_case_puts_its_edge_queries_behind_the_first_chunk():
    c = hc.case("chunked")
    nq = len(c["queries"])
    assert nq > 2 * hc.SLOTS and nq % hc.SLOTS != 0 and nq == 2 * hc.SLOTS + 5  # a ragged last chunk
    no_token = [q for q in range(nq) if not c["queries"][q]]
    no_list = [q for q in range(nq) if c["counts"][q] == 0]
    assert any(q >= hc.SLOTS for q in no_token) and any(q >= hc.SLOTS for q in no_list)
    assert any(q >= 2 * hc.SLOTS for q in no_token)  # one of them in the ragged last chunk
    assert all(len(hc.positives(c, q)) > 0 for q in range(nq) if q not in no_token)
    assert len({tuple(q) for q in c["queries"]}) > nq // 2  # a slot's next query is another query
