"""-m gpu: the forms of the row-screen kernels (search.cuh, beam_search_screen_kernel<3, 4> and <6, 2>) that test_gpu_row_screen.py
and test_gpu_row_screen_wide.py never launch: plane rows with a 64-element tail (one block + tail, two blocks + tail), the <6, 2> form
over lists of 64 ids, Vamana handles, queries whose visited set leaves LDS inside the screen kernel, the batch threshold itself, a
beam of one, rows and queries far off unit norm, rows with an infinity in them, and a composite handle.

Bar per case, unless the case says otherwise: ids, distance bits, counts and the three visit counters equal with the screen on, with it
off, and in the oracle walking the same graph; the device's ruled-out total equal to the oracle's count of the rows its restatement of
the bound (oracle.c: orc_screen_lb, held to row_screen.h by tests/test_cpu_row_screen.py) rules out on that walk; nothing counted with
the screen off.  "count > 0" is asked of the ORACLE's count, so no case passes by screening nothing.  n = 3000 two-cluster rows, 704
queries, k = 10 unless a case says otherwise."""
import numpy as np
import pytest

import test_gpu_row_screen_wide as wide
from test_gpu_row_screen import NQ, _built, _on_off, _same, _same_as_oracle, _search_counted
from util import synth

pytestmark = pytest.mark.gpu

N = 3000
M = 16


def _rows(po, d, n=N, nq=NQ):
    return synth(po, n, d, n_clusters=2), synth(po, nq, d, stream=1, n_clusters=2)


def _oracle_graph(po, X, g):
    return po.Graph.from_arrays(X, g["M"], g["M0"], g["max_level"], g["entry"], g["levels"], g["upper_off"], g["adj0"], g["adjU"])


def _handle(la, kind, X, g):
    return la.BackendSearcher.from_arrays(kind, X, g["M"], g["M0"], g["max_level"], g["entry"], g["levels"], g["upper_off"], g["adj0"], g["adjU"])


def _bar(s, G, Q, k, ef, algo=0, positive=True, what=""):
    """the full bar; returns the screen-on leg and the oracle's count"""
    on, off = _on_off(s, Q, k, ef)
    evals = on["stats"]["n_dist_evals"] - len(Q)
    print(f"{what} nq={len(Q)} k={k} ef={ef}: ruled out {on['ruled']} of {evals} evaluations, read in full {on['full']}")
    _same(on, off)
    want = _same_as_oracle(on, G, Q, k, ef, algo)  # answers, visit counters, and ruled out == the oracle's count
    assert on["ruled"] + on["full"] == evals
    assert off["ruled"] == 0 and off["full"] == 0
    if positive:
        assert want > 0, "the oracle rules nothing out here: the case shows nothing"
    return on, want


# ---- plane shapes ----------------------------------------------------------------------------------------------------------------------
# 516: T = 3, plane rows of 576 = one interleaved block + a 64-element tail that holds 4 elements; 1028: T = 5 in the 6-kernel, plane
# rows of 1088 = two interleaved blocks + a 64-element tail, and the sixth chunk lies wholly past the plane row (plane_tail_load's zeros)
@pytest.mark.parametrize("d", [516, 1028])
def test_plane_rows_with_a_64_element_tail(la, po, gpu, d):
    X, Q = _rows(po, d)
    s, G, dX = _built(la, po, X)
    for ef in (10, 56):
        _bar(s, G, Q, 10, ef, what=f"d={d} M={M}")
    s.close()


def test_six_chunk_form_over_lists_of_64(la, po, gpu):
    """d = 1100 at M = 32: <6, 2> evaluates 8 rows per round, a level-0 list of 64 ids takes up to 8 rounds of one hop"""
    d = 1100
    X, Q = _rows(po, d)
    s, G, dX = wide._built(la, po, X)
    assert int((s.graph_export()["adj0"] != 0xFFFFFFFF).sum(1).max()) > 32  # lists longer than any M = 16 graph has
    _bar(s, G, Q, 10, 56, what=f"d={d} M=32")
    s.close()


# ---- Vamana ----------------------------------------------------------------------------------------------------------------------------
# one level, lists of R ids, the sorted-list GreedySearch in the oracle (algo 1).  R = 64: several hi rounds per hop in <3, 4> (28 rows a
# round), 8 rounds in <6, 2>
@pytest.mark.parametrize("R,d", [(32, 768), (64, 768), (32, 1100)])
def test_vamana_handle_is_screened(la, po, gpu, R, d):
    X, Q = _rows(po, d)
    dX = la.DeviceArray.from_host(X)
    s = la.BackendSearcher.build_device(la.BackendType.DiskAnn, dX.ptr, N, d, d, R, 64)
    g = s.graph_export()
    assert g["max_level"] == 0 and g["M0"] == R
    _bar(s, _oracle_graph(po, X, g), Q, 10, 56, algo=1, what=f"vamana R={R} d={d}")
    s.close()


# ---- the visited set leaves LDS inside the screen kernel -------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [768, 1100])
def test_visited_set_moves_to_hbm_inside_the_screen_kernel(la, po, gpu, monkeypatch, d):
    """A 256-slot LDS table (it is left at 75 % load): every query of the batch evaluates more rows than that, so each one migrates to
    an HBM pool table in mid-walk and redoes the hop that found the table full (hop_migrate.cuh).  The redone hop's rows are screened
    once: the ruled-out total is still the oracle's, which knows nothing of tables."""
    X, Q = _rows(po, d)
    s, G, dX = _built(la, po, X)  # built with the table the builder would have anyway; the knob is read by every search
    monkeypatch.setenv("LEANN_DEBUG_HASH_BITS", "8")
    la.lib().leann_debug_reload_env()
    ost = G.search_batch(Q, 10, 56, 0, nthreads=8)[3]
    assert int(ost[:, 0].min()) > 256  # on the oracle's numbers: no query fits the table
    on, want = _bar(s, G, Q, 10, 56, what=f"d={d}, 256 slots")
    assert on["stats"]["n_table_overflow"] >= NQ
    s.close()


# ---- the batch threshold ---------------------------------------------------------------------------------------------------------------
def test_batch_threshold_641(la, po, gpu):
    """641 queries: the 4-wave form, screened.  640 and 384 on the same handle with the screen on: the 8- and 16-wave forms read whole
    rows — both counters stay where they were — and answer as the oracle does."""
    d = 768
    X, Q = _rows(po, d)
    s, G, dX = _built(la, po, X)
    _bar(s, G, Q[:641], 10, 56, what="threshold")
    s.set_row_screen(True)
    for nq in (640, 384):
        r = _search_counted(s, Q[:nq], 10, 56)
        assert r["ruled"] == 0 and r["full"] == 0, nq
        ok, od, oc, ost = G.search_batch(Q[:nq], 10, 56, 0, nthreads=8)
        assert (r["counts"] == oc).all() and (r["keys"] == ok).all() and (r["dists"].view(np.uint32) == od.view(np.uint32)).all(), nq
        for i, f in enumerate(("n_dist_evals", "n_hops_base", "n_hops_upper")):
            assert r["stats"][f] == int(ost[:, i].sum()), (nq, f)
    s.close()


# ---- the smallest beam -----------------------------------------------------------------------------------------------------------------
def test_beam_of_one(la, po, gpu):
    """k = 1, ef = 1: a beam of one is full from the first hop on every level, level 0 included — every evaluated row but the entry
    point's is screened against the best distance so far"""
    d = 768
    X, Q = _rows(po, d)
    s, G, dX = _built(la, po, X)
    _bar(s, G, Q, 1, 1, what="beam of one")
    s.close()


# ---- rows and queries off unit norm ----------------------------------------------------------------------------------------------------
# The graph is built on the clean rows and reused over the scaled ones (from_arrays), so the builder plays no part.
@pytest.mark.parametrize("sx,sq,positive", [(37.5, 1e-3, True), (1e-30, 1e-10, False)])
def test_off_unit_norm(la, po, gpu, sx, sq, positive):
    """x 37.5 / x 1e-3: dot products of about 0.04, nothing about the bound assumes norm 1.  x 1e-30 / x 1e-10: every product is
    subnormal or zero, every distance is 1.0, ties run by key, and of the bound only the absolute term E (row_screen.h (5)) is left:
    1 - (U + E) rounds to 1.0, which is not above a worst distance of 1.0, so the oracle rules nothing out — and neither may the
    device, whether it keeps subnormals or flushes them (the proof covers both)."""
    d = 768
    X, Q = _rows(po, d)
    s0, G0, dX = _built(la, po, X)
    g = s0.graph_export()
    s0.close()
    Xs, Qs = X * np.float32(sx), Q * np.float32(sq)
    s = _handle(la, la.BackendType.Hnsw, Xs, g)
    G = _oracle_graph(po, Xs, g)
    on, want = _bar(s, G, Qs, 10, 56, positive=positive, what=f"rows x {sx:g}, queries x {sq:g}")
    if not positive:
        assert (on["dists"][on["keys"] != np.iinfo(np.uint64).max] == 1.0).all()
    s.close()


# ---- infinities ------------------------------------------------------------------------------------------------------------------------
def test_rows_with_an_infinity_take_the_whole_row_path(la, po, gpu):
    """One +inf or -inf element in about 1 % of the rows, in columns where no query element is zero: such a row's distance is -inf or
    +inf, its lower bound -inf or NaN, `lb > worst` false — it is read in full whatever the beam holds, and is counted so.  (NaN
    elements are out of scope: NaN payloads differ between host and device, a bit comparison would test the hosts.)"""
    d = 768
    X, Q = _rows(po, d)
    s0, G0, dX = _built(la, po, X)
    g = s0.graph_export()
    s0.close()
    cols = np.flatnonzero((Q != 0).all(axis=0))
    assert len(cols) >= 8
    rng = np.random.default_rng(11)
    bad = rng.choice(N, N // 100, replace=False)
    Xp = X.copy()
    Xp[bad, rng.choice(cols, len(bad))] = np.where(rng.random(len(bad)) < 0.5, np.float32(np.inf), np.float32(-np.inf))
    assert np.isinf(Xp).sum() == len(bad) and not np.isnan(Xp).any()
    for i in bad:  # the reference's own view of a poisoned row: never above any worst distance
        assert not (po.screen_lb(Q[0], Xp[i]) > -np.inf)
        assert np.isinf(po.dist_canon(Q[0], Xp[i]))
    s = _handle(la, la.BackendType.Hnsw, Xp, g)
    G = _oracle_graph(po, Xp, g)
    on, want = _bar(s, G, Q, 10, 56, what="1 % of the rows hold an infinity")
    assert np.isin(on["keys"], bad.astype(np.uint64)).any()  # poisoned rows are reached, and returned (those at -inf)
    s.close()


# ---- composite handle ------------------------------------------------------------------------------------------------------------------
def test_two_shard_composite_is_screened(la, po, gpu):
    """Two shards on one device, the screen switched on through the composite handle (include/leann_backend.h: "Works on composite
    handles"): every shard walks all 704 queries with the same k and ef, so the composite's counters move by the sum of the oracle's
    counts over the two exported shard graphs; switched off through the same handle, they stop."""
    d, k, ef = 768, 10, 56
    n = 4000
    X, Q = _rows(po, d, n=n)
    lows = [0, 2000, n]
    parts = [la.DeviceArray.from_host(X[lows[i]:lows[i + 1]]) for i in range(2)]
    sh = la.ShardedIndex.build_device(la.BackendType.Hnsw, [p.ptr for p in parts], [lows[i + 1] - lows[i] for i in range(2)], d, d, M, 64,
                                      [0, 0], keep=parts)
    s = sh.as_backend()
    assert s.n_shards() == 2
    want = 0
    for i in range(2):
        G = _oracle_graph(po, X[lows[i]:lows[i + 1]], s.shard(i).graph_export())
        want += int(G.search_counted_batch(Q, k, ef, 0, nthreads=8)[4].sum())
    assert want > 0
    on, off = _on_off(s, Q, k, ef)
    print(f"composite: ruled out {on['ruled']}, read in full {on['full']}; oracle {want}")
    assert (on["counts"] == off["counts"]).all() and (on["keys"] == off["keys"]).all()
    assert (on["dists"].view(np.uint32) == off["dists"].view(np.uint32)).all()
    assert (on["counts"] == k).all()
    assert on["ruled"] == want
    assert off["ruled"] == 0 and off["full"] == 0
    s.close()
    sh.close()
