"""-m gpu: the split-plane row screen of the throughput beam search (csrc/row_screen.h, planes.hip, search.cuh).  Batches of more than
640 unfiltered queries read a neighbour's upper 16-bit halves first and its lower halves only if a proved lower bound does not put it
behind the full beam.  Bar: ids, distance bits, counts and stats equal with the screen on, with it off, and in the oracle walking the
exported graph; and the number of rows the device ruled out equals, exactly, the number the oracle's restatement of the decision
(oracle.c: orc_screen_lb, the counting search) rules out on the same walk.  A bound that is too weak changes no answer, only that count;
one that is too strong changes it too, whether or not the wrongly dropped row would have entered a beam."""
import numpy as np
import pytest

from util import SEED, synth

pytestmark = pytest.mark.gpu

NQ = 704  # more than 640: the 4-wave (throughput) form, the only one that screens
M = 16


def _built(la, po, X):
    """index built on the GPU from rows in HBM + the oracle's view of the exported graph"""
    n, d = X.shape
    dX = la.DeviceArray.from_host(X)
    s = la.BackendSearcher.build_device(la.BackendType.Hnsw, dX.ptr, n, d, d, M, 64)
    g = s.graph_export()
    G = po.Graph.from_arrays(X, M, 2 * M, g["max_level"], g["entry"], g["levels"], g["upper_off"], g["adj0"], g["adjU"])
    return s, G, dX


def _on_off(s, Q, k, ef):
    """one search with the screen on, one with it off; the counters' increments of each"""
    out = []
    for enable in (True, False):
        s.set_row_screen(enable)
        c0 = s.row_screen_stats()
        s.stats(reset=True)
        keys, dists, counts = s.search_batch(Q, k, ef)
        c1 = s.row_screen_stats()
        out.append(dict(keys=keys, dists=dists, counts=counts, stats=s.stats(),
                        ruled=c1["ruled_out"] - c0["ruled_out"], full=c1["read_in_full"] - c0["read_in_full"]))
    s.set_row_screen(True)
    return out


def _same(a, b):
    assert (a["counts"] == b["counts"]).all()
    assert (a["keys"] == b["keys"]).all(), f"ids differ in {(a['keys'] != b['keys']).any(axis=1).sum()} queries"
    assert (a["dists"].view(np.uint32) == b["dists"].view(np.uint32)).all()
    for f in ("n_dist_evals", "n_hops_base", "n_hops_upper"):
        assert a["stats"][f] == b["stats"][f], f


def _same_as_oracle(a, G, Q, k, ef, algo=0):
    """answers and visit counters as the oracle's, and the device's ruled-out total as the oracle's count; returns that count"""
    ok, od, oc, ost, oruled = G.search_counted_batch(Q, k, ef, algo, nthreads=8)
    assert (a["counts"] == oc).all()
    assert (a["keys"] == ok).all(), f"ids differ from the oracle's in {(a['keys'] != ok).any(axis=1).sum()} queries"
    assert (a["dists"].view(np.uint32) == od.view(np.uint32)).all()
    assert a["stats"]["n_dist_evals"] == int(ost[:, 0].sum())
    assert a["stats"]["n_hops_base"] == int(ost[:, 1].sum())
    assert a["stats"]["n_hops_upper"] == int(ost[:, 2].sum())
    assert a["ruled"] == int(oruled.sum()), f"ruled out: device {a['ruled']}, oracle {int(oruled.sum())}"
    return int(oruled.sum())


# 1100: T = 5 in the 6-kernel, plane rows of 1152 (two interleaved blocks + a 128-element tail, the sixth chunk reads as zeros);
# 1280: T = 5 with the tail chunk exactly full; 520: T = 3, plane rows of 576 (one interleaved block + a 64-element tail)
@pytest.fixture(scope="module", params=[768, 1536, 700, 1100, 1280, 520])
def clustered(request, la, po, gpu):
    d = request.param
    X = synth(po, 4000, d, n_clusters=2)  # two clusters: beams fill with one cluster's rows, the other's are ruled out
    Q = synth(po, NQ, d, stream=1, n_clusters=2)
    s, G, dX = _built(la, po, X)
    yield s, G, Q
    s.close()


@pytest.mark.parametrize("ef", [10, 56, 200])
def test_screen_on_equals_off_equals_oracle(clustered, ef):
    s, G, Q = clustered
    on, off = _on_off(s, Q, 10, ef)
    print(f"d={Q.shape[1]} ef={ef}: ruled out {on['ruled']}, read in full {on['full']}, evals {on['stats']['n_dist_evals']}")
    _same(on, off)
    _same_as_oracle(on, G, Q, 10, ef)
    assert on["ruled"] > 0
    assert on["ruled"] + on["full"] == on["stats"]["n_dist_evals"] - NQ  # every evaluation but each query's entry point
    assert off["ruled"] == 0 and off["full"] == 0                        # the whole-row kernel counts nothing


def test_adversarial_rows_at_the_bound(la, po, gpu):
    """Near-duplicates of one direction: every distance sits within about 1e-3 of the beam's threshold.  The lower halves are forced
    to the worst case of the truncation (0xFFFF where the element has the query's sign, 0 elsewhere), a few elements are zero or
    subnormal.  A bound that promised a hair too much would rule out a row that belongs in the beam."""
    n, d = 2048, 768
    rng = np.random.default_rng(SEED)
    c = rng.standard_normal(d)
    c /= np.linalg.norm(c)

    def near(m):
        v = c + 1e-3 * rng.standard_normal((m, d))
        return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)

    X, Q = near(n), near(NQ)
    bits = X.view(np.uint32)
    same_sign = (bits >> 31).astype(bool) == (Q[0] < 0)[None, :]
    bits[:] = (bits & np.uint32(0xFFFF0000)) | np.where(same_sign, np.uint32(0xFFFF), np.uint32(0))
    for j, b in ((5, 0x00000000), (77, 0x80000000), (300, 0x0000FFFF), (511, 0x807FFFFF), (767, 0x0080FFFF)):
        bits[j::9, j] = np.uint32(b)  # zeros, subnormals, the smallest normal
    s, G, dX = _built(la, po, X)
    for ef in (10, 56):
        on, off = _on_off(s, Q, 10, ef)
        print(f"adversarial ef={ef}: ruled out {on['ruled']}, read in full {on['full']}")
        _same(on, off)
        _same_as_oracle(on, G, Q, 10, ef)
        assert on["ruled"] + on["full"] == on["stats"]["n_dist_evals"] - NQ
    s.close()


def _search_counted(s, Q, k, ef):
    """one search as the handle stands (no set_row_screen call) + the counters' increments"""
    c0 = s.row_screen_stats()
    s.stats(reset=True)
    keys, dists, counts = s.search_batch(Q, k, ef)
    c1 = s.row_screen_stats()
    return dict(keys=keys, dists=dists, counts=counts, stats=s.stats(),
                ruled=c1["ruled_out"] - c0["ruled_out"], full=c1["read_in_full"] - c0["read_in_full"])


def test_planes_are_cut_when_a_handle_is_made(la, po, gpu, monkeypatch):
    """LEANN_ROW_SCREEN=1: build_device and from_arrays cut the planes themselves — the first search screens with no call to
    set_row_screen — and agree with the oracle.  =0: no planes, nothing counted.  Unset: an index this small (12 MB of rows, under the
    1 GiB of the automatic mode) keeps none either."""
    d = 768
    X = synth(po, 4000, d, n_clusters=2)
    Q = synth(po, NQ, d, stream=1, n_clusters=2)
    monkeypatch.setenv("LEANN_ROW_SCREEN", "1")
    la.lib().leann_debug_reload_env()
    s, G, dX = _built(la, po, X)
    g = s.graph_export()
    t = la.BackendSearcher.from_arrays(la.BackendType.Hnsw, X, M, 2 * M, g["max_level"], g["entry"], g["levels"], g["upper_off"], g["adj0"], g["adjU"])
    monkeypatch.setenv("LEANN_ROW_SCREEN", "0")
    la.lib().leann_debug_reload_env()
    off = la.BackendSearcher.from_arrays(la.BackendType.Hnsw, X, M, 2 * M, g["max_level"], g["entry"], g["levels"], g["upper_off"], g["adj0"], g["adjU"])
    monkeypatch.delenv("LEANN_ROW_SCREEN")
    la.lib().leann_debug_reload_env()  # the mode is a property of the handle from here on
    auto = la.BackendSearcher.from_arrays(la.BackendType.Hnsw, X, M, 2 * M, g["max_level"], g["entry"], g["levels"], g["upper_off"], g["adj0"], g["adjU"])
    a, b, c, e = (_search_counted(h, Q, 10, 56) for h in (s, t, off, auto))
    for r in (a, b):
        assert r["ruled"] > 0 and r["ruled"] + r["full"] == r["stats"]["n_dist_evals"] - NQ
        _same_as_oracle(r, G, Q, 10, 56)
    for r in (c, e):
        assert r["ruled"] == 0 and r["full"] == 0
        _same(r, a)
    for h in (s, t, off, auto):
        h.close()


def test_planes_follow_appended_and_removed_rows(la, po, gpu, tmp_path, monkeypatch):
    """add_to_index, then a removal with consolidation.  The handle is opened with LEANN_ROW_SCREEN=1, so its planes are cut by the open
    itself, from the file add_to_index wrote: the first search screens (ruled out > 0 before any set_row_screen call), returns appended
    rows, and agrees with the whole-row path; so do the searches after the removal and the repair.  Both times the oracle walks the graph
exported at that moment and its count of ruled-out rows is the device's."""
    d, n_old, n_add = 768, 3000, 1000
    X = synth(po, n_old + n_add, d, n_clusters=2)
    Q = synth(po, NQ, d, stream=1, n_clusters=2)
    stem = str(tmp_path / "documents.leann")
    monkeypatch.setenv("LEANN_ROW_SCREEN", "1")
    la.lib().leann_debug_reload_env()
    b = la.BackendBuilder(la.BackendType.Hnsw)
    b.build(X[:n_old], [], stem, d, M, 64)
    b.add_to_index(X[n_old:], stem, d, n_old)
    s = la.BackendSearcher.load(la.BackendType.Hnsw, stem, d)
    assert s.len() == n_old + n_add
    on = _search_counted(s, Q, 10, 56)
    assert on["ruled"] > 0 and on["ruled"] + on["full"] == on["stats"]["n_dist_evals"] - NQ
    assert (on["keys"] >= n_old).any()  # appended rows are among the answers
    g = s.graph_export()
    _same_as_oracle(on, po.Graph.from_arrays(X, M, 2 * M, g["max_level"], g["entry"], g["levels"], g["upper_off"], g["adj0"], g["adjU"]), Q, 10, 56)
    s.set_row_screen(False)
    off = _search_counted(s, Q, 10, 56)
    assert off["ruled"] == 0 and off["full"] == 0
    _same(on, off)
    gone = np.unique(on["keys"][:, 0])[::2].astype(np.uint64)  # half of the nearest neighbours
    assert s.remove(gone) == len(gone)
    s.consolidate()
    off = _search_counted(s, Q, 10, 56)
    s.set_row_screen(True)  # the planes cut at the open are still the handle's: rows do not move under a removal or a repair
    on = _search_counted(s, Q, 10, 56)
    _same(on, off)
    assert off["ruled"] == 0 and on["ruled"] > 0 and on["ruled"] + on["full"] == on["stats"]["n_dist_evals"] - NQ
    assert not np.isin(on["keys"], gone).any()
    g = s.graph_export()  # after the repair no live list names a removed row: the plain walk of the export is the search
    _same_as_oracle(on, po.Graph.from_arrays(X, M, 2 * M, g["max_level"], g["entry"], g["levels"], g["upper_off"], g["adj0"], g["adjU"]), Q, 10, 56)
    s.close()
