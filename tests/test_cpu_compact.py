"""Compaction's numpy restatement (tests/compact_ref.py) held to a graph written out by hand and to the property that makes compaction
a pure renaming: oracle walks of the compacted arrays return, through new_to_old, what walks of the consolidated arrays return —
keys, f32 distance bits, counts and the three counters.  No device: this pins the reference, not the product."""
import numpy as np
import pytest

import compact_ref as cp
import consolidate_ref as cr

E = cp.EMPTY


def test_six_nodes_by_hand():
    """positions 1 and 4 are removed (already unreachable); levels 0 2 1 0 1 1 -> upper lists: node 1 {0, 1}, node 2 {2}, node 4 {3},
    node 5 {4}.  Old -> new: 0->0, 2->1, 3->2, 5->3."""
    X = (np.arange(6 * 4, dtype=np.float32).reshape(6, 4) / 8).astype(np.float32)
    g = dict(kind="hnsw", X=X, M=2, M0=3, max_level=1, entry=2,
             levels=np.array([0, 2, 1, 0, 1, 1], np.uint8), upper_off=np.array([0, 0, 2, 3, 3, 4], np.uint32),
             adj0=np.array([[2, 3, E], [E, E, E], [0, E, 5], [5, 0, 2], [E, E, E], [E, 3, E]], np.uint32),
             adjU=np.array([[E, E], [E, E], [5, E], [E, E], [E, 2]], np.uint32))
    removed = np.array([0, 1, 0, 0, 1, 0], bool)
    out, m = cp.compact(g, removed)
    assert m.tolist() == [0, 2, 3, 5]
    assert (out["X"] == X[[0, 2, 3, 5]]).all()
    assert out["levels"].tolist() == [0, 1, 0, 1] and out["upper_off"].tolist() == [0, 0, 1, 1]
    assert out["adj0"].tolist() == [[1, 2, E], [0, E, 3], [3, 0, 1], [E, 2, E]]
    assert out["adjU"].tolist() == [[3, E], [E, 1]]
    assert out["entry"] == 1 and out["max_level"] == 1 and out["M"] == 2 and out["M0"] == 3 and out["kind"] == "hnsw"
    # the input is left alone, and an unconsolidated graph is refused
    assert g["adj0"][0].tolist() == [2, 3, E] and g["entry"] == 2
    g["adj0"][0, 2] = 4
    with pytest.raises(AssertionError):
        cp.compact(g, removed)
    g["adj0"][0, 2] = E
    with pytest.raises(AssertionError):
        cp.compact(g, np.array([0, 0, 1, 0, 0, 0], bool))   # the entry point


def removal_pattern(rng, g):
    """about 30 % at random plus the entry, positions 0 and n - 1, a run of 160 consecutive positions, every second position of
    another stretch and some nodes of level >= 1"""
    n = len(g["X"])
    removed = rng.random(n) < 0.25
    removed[[g["entry"], 0, n - 1]] = True
    removed[n // 3: n // 3 + 160] = True
    removed[n // 2: n // 2 + 200: 2] = True
    removed[n // 2 + 1: n // 2 + 200: 2] = False
    removed[np.flatnonzero(g["levels"] >= 1)[:12]] = True
    return removed


SHAPES = {"hnsw_2085": ("hnsw", 2085, 40, 8, 16, 2), "hnsw_3001": ("hnsw", 3001, 24, 4, 8, 3), "vamana_r96_1500": ("diskann", 1500, 72, 96, 96, 0)}


@pytest.mark.parametrize("name", list(SHAPES))
def test_walks_of_the_compacted_graph_are_the_walks_of_the_consolidated_one(po, name):
    kind, n, d, M, M0, ml = SHAPES[name]
    rng = np.random.default_rng(len(name) + n)
    g = cr.random_graph(rng, kind, n, d, M, M0, ml)
    removed = removal_pattern(rng, g)
    assert removed[g["entry"]] and removed[0] and removed[n - 1] and 0.2 < removed.mean() < 0.45
    c = cr.consolidate(g, removed)
    assert cr.pending(c, removed) == 0
    k, m = cp.compact(c, removed)
    live = n - int(removed.sum())
    assert len(m) == live == len(k["X"]) and (np.diff(m) > 0).all() and not removed[m].any()
    assert int(k["levels"].astype(np.int64).sum()) == len(k["adjU"])
    algo = 0 if kind == "hnsw" else 1
    Q = (rng.integers(-2, 3, (64, d)) / 8.0).astype(np.float32)

    def oracle(gr):
        return po.Graph.from_arrays(gr["X"], gr["M"], gr["M0"], gr["max_level"], gr["entry"], gr["levels"], gr["upper_off"], gr["adj0"],
                                    gr["adjU"] if len(gr["adjU"]) else np.full((1, gr["M"]), E, np.uint32))

    Gc, Gk = oracle(c), oracle(k)
    for ef in (10, 48):
        ck, cd, cc, cs = Gc.search_batch(Q, 10, ef, algo, nthreads=4)
        kk, kd, kc, ks = Gk.search_batch(Q, 10, ef, algo, nthreads=4)
        assert (cc == kc).all() and (cc > 0).all() and (cs == ks).all()
        assert (cd.view(np.uint32) == kd.view(np.uint32)).all()
        for i in range(len(Q)):
            assert (m[kk[i, : kc[i]].astype(np.int64)] == ck[i, : cc[i]].astype(np.int64)).all()
            assert not removed[ck[i, : cc[i]].astype(np.int64)].any()
