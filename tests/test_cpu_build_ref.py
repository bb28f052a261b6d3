"""CPU: the batched builder's restatement (tests/build_ref.py) and the oracle's construction search, checked without the code under
test — test_gpu_build_parity.py then holds csrc/build.hip to this restatement list for list."""
import numpy as np
import pytest

import build_ref as br
import consolidate_ref as cr
from util import recall_at_k, synth


def test_search_level_at_level_0_is_the_plain_search(po):
    n, d, M, ef = 2000, 32, 8, 40
    X = synth(po, n, d)
    Q = synth(po, 20, d, stream=1)
    for G, algo in ((po.Graph.build_hnsw(X, M=M, efc=48), 0), (po.Graph.build_vamana(X, R=12, L=32), 1)):
        for q in Q:
            keys, exp = G.search_level(q, 0, ef, algo, exp_cap=256)
            k0, d0, _ = G.search(q, ef, ef, algo)
            assert ((keys & br.LOW) == k0).all() and (br.orderable_f32((keys >> br.S32).astype(np.uint32)) == d0).all()
            assert (keys[1:] > keys[:-1]).all()
            assert len(exp) >= 1 and len(set((exp & br.LOW).tolist())) == len(exp)  # a node is expanded once
            assert set((keys & br.LOW).tolist()) <= set((exp & br.LOW).tolist())   # the walk ends when the whole beam is expanded
            assert (G.search_level(q, 0, ef, algo, exp_cap=3)[1] == exp[:3]).all()
    G = po.Graph.build_hnsw(X, M=M, efc=48)
    assert G.max_level >= 2
    q = Q[0]
    for level in range(1, G.max_level + 1):
        keys, _ = G.search_level(q, level, ef, 0)
        levels = G.export()[0]
        assert len(keys) and (levels[(keys & br.LOW).astype(np.int64)] >= level).all()
    keys, exp = G.search_level(q, G.max_level + 1, ef, 0, exp_cap=8)
    assert len(keys) == 0 and len(exp) == 0  # the kernel's level loop does not run
    rows = np.array([5, 77, 1999], np.uint32)
    bk, bc, be, bn = G.search_level_batch(rows, 1, ef, 0, exp_cap=16, nthreads=2)
    for i, r in enumerate(rows):
        keys, exp = G.search_level(X[r], 1, ef, 0, exp_cap=16)
        assert bc[i] == len(keys) and (bk[i, : bc[i]] == keys).all() and bn[i] == len(exp) and (be[i, : bn[i]] == exp).all()


def test_insertion_order():
    for lo, n in ((0, 1), (0, 1000), (300, 1000), (1000, 1000)):
        o = br.insertion_order(lo, n)
        assert sorted(o.tolist()) == list(range(n)) and (o[:lo] == np.arange(lo)).all()
    o = br.insertion_order(0, 1000)
    assert (o[:20] != np.arange(20)).any()
    p = br.insertion_order(0, 1000, pin_first=617)
    assert p[0] == 617 and sorted(p.tolist()) == list(range(1000)) and (p[1:] == o[o != 617]).all()
    # position-hash order: the rows [lo, n) come in the order their positions have in a build of all n rows
    assert (br.insertion_order(300, 1000)[300:] == o[o >= 300]).all()


def test_batch_sizes():
    assert br.batch_sizes(1, 400, 1 << 20) == [1] * 399  # fraction at its maximum: one point per batch
    assert br.batch_sizes(1, 400, 1) == [1, 2, 4, 8, 16, 32, 64, 128, 144]
    assert br.batch_sizes(1, 100, 8)[:9] == [1] * 9 and sum(br.batch_sizes(1, 100, 8)) == 99
    assert br.batch_sizes(800, 1200, 8) == [100, 112, 126, 62]
    assert br.batch_sizes(0, 800, 8, refine=True) == [800]
    assert br.batch_sizes(1, 200_000, 8)[-2] == br.BMAX


@pytest.mark.parametrize("name", list(br.CASES))
def test_case_graph_is_valid_and_takes_its_paths(po, name):
    c = br.CASES[name]
    g = br.case_graph(po, name)
    assert not br.check_lists(g), br.check_lists(g)
    assert ((g["adj0"] != br.EMPTY).sum(1) >= 1).all()
    cn = g["counters"]
    assert all(cn[k] > 0 for k in c["need"]) and all(cn[k] == 0 for k in c["zero"]), cn
    if c["kind"] == br.VA and "LEANN_VAMANA_NAV" not in c["knobs"]:
        first, gap = br.medoid(br.case_rows(c))
        assert gap >= 1e-6 and g["entry"] == first and g["max_level"] == 0
    else:
        assert g["max_level"] == int(g["levels"].max()) and g["levels"][g["entry"]] == g["max_level"]
    if name == "hnsw_fraction_max":
        assert g["batches"] == [1] * (c["n"] - 1)
    if name == "hnsw_fraction_1":
        assert g["batches"] == br.batch_sizes(1, c["n"], 1) and max(g["batches"]) > c["n"] // 4


def test_grid_rows_are_exact():
    for shape in ("uniform", "hubs", "blocks"):
        X = br.grid_rows(7, 300, 128, shape)
        assert (np.abs(X * 8) <= 4).all() and (X * 8 == np.round(X * 8)).all()
        G32 = X @ X.T  # any summation order
        assert (G32 == (X.astype(np.float64) @ X.astype(np.float64).T)).all()


@pytest.mark.parametrize("name", ["hnsw_fraction_1", "vamana_two_pass"])
def test_c_prune_is_the_numpy_prune(po, name):
    """oracle.c:orc_prune carries the restatement's hot loop; consolidate_ref.prune (numpy) is the rule's one statement"""
    c = br.CASES[name]
    X = br.case_rows(c, 300)
    a = br.BuildRef(po, c["kind"], X, c["M"], c["efc"], c["knobs"]).build()
    b = br.BuildRef(po, c["kind"], X, c["M"], c["efc"], c["knobs"], numpy_prune=True).build()
    assert (a["adj0"] == b["adj0"]).all() and (a["adjU"] == b["adjU"]).all() and a["counters"] == b["counters"]
    rng = np.random.default_rng(3)
    for alpha, ts in ((0.0, False), (1.2, False), (1.2, True), (1.0, True)):
        for _ in range(20):
            ids = rng.choice(300, 60, replace=False).astype(np.uint32)
            dd = (np.float32(1.0) - X[ids] @ X[0]).astype(np.float32)
            o = np.lexsort((ids, dd))
            assert po.prune(X, ids[o], dd[o], 24, alpha, ts).tolist() == list(cr.prune(X, ids[o].astype(np.int64), dd[o], 24, alpha, ts))


def test_continue_from_an_empty_tail_changes_nothing(po):
    c = br.CASES["hnsw_m8"]
    X = br.case_rows(c, 300)
    g = br.BuildRef(po, br.HN, X, c["M"], c["efc"]).build()
    h = br.BuildRef(po, br.HN, X, c["M"], c["efc"]).continue_from(g, 300)
    assert (g["adj0"] == h["adj0"]).all() and (g["adjU"] == h["adjU"]).all() and h["entry"] == g["entry"]
    h = br.BuildRef(po, br.HN, br.case_rows(c, 400), c["M"], c["efc"]).continue_from(g, 300)
    assert not br.check_lists(h) and h["batches"] == br.batch_sizes(300, 400, 8)


def test_restatement_is_a_builder(po):
    """normalised rows, 3000 x 64: the restatement's graphs, searched by the oracle, reach the recall of the oracle's sequential
    builders within 0.01 at ef 32 and 64 — the bar test_gpu_builder_quality.py sets for the device builder"""
    n, d = 3000, 64
    X = synth(po, n, d)
    Q = synth(po, 200, d, stream=1)
    truth = po.exact_topk(X, Q, 10)
    for kind, M, efc, algo, seq in ((br.HN, 16, 64, 0, po.Graph.build_hnsw(X, M=16, efc=64)),
                                    (br.VA, 32, 64, 1, po.Graph.build_vamana(X, R=32, L=64, alpha=1.2))):
        g = br.BuildRef(po, kind, X, M, efc).build()
        assert not br.check_lists(g)
        G = po.Graph.from_arrays(X, g["M"], g["M0"], g["max_level"], g["entry"], g["levels"], g["upper_off"], g["adj0"], g["adjU"])
        for ef in (32, 64):
            r_seq = recall_at_k(seq.search_batch(Q, 10, ef, algo, nthreads=4)[0], truth)
            r_ref = recall_at_k(G.search_batch(Q, 10, ef, algo, nthreads=4)[0], truth)
            print(f"{kind} ef={ef}: recall@10 sequential {r_seq:.4f} / restatement {r_ref:.4f}")
            assert r_ref >= r_seq - 0.01
