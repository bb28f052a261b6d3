"""-m gpu: every way of making a handle stages its rows through one function (csrc/handle.hip) — held here at a `dims` that is no
multiple of 4 (d = 30: ld = 32, two padding floats per row, which must be +0.0) and at one that is (d = 32: the branch without
padding).  n = 600, HNSW M = 8 / efc = 32 unless a case says otherwise; rows from util.synth.

Before each case a device block larger than the rows is filled with NaN and freed, so that the handle's block is likely (not
certainly) recycled memory; no assertion depends on that.  f32 handles: the device rows, downloaded whole, hold the input bit for
bit in the data columns and +0.0 in the padding.  bf16 handles: the exported rows are round_bf16(X).  Every handle: 16 queries
return the ids and distance bits of the oracle walking the exported graph.

The last test holds what a derived handle takes from its source: the prune form through append and compact, removals through
to_rows."""

import numpy as np
import pytest

import consolidate_ref as cr
from test_gpu_compact import _graph_dict
from test_gpu_delete import _searcher
from test_gpu_delete_edges import _round
from test_gpu_dropin import _stock_dir
from util import synth

pytestmark = pytest.mark.gpu

N, M, EFC, K, EF = 600, 8, 32, 5, 40
DIMS = (30, 32)


def _rows(po, n, d, stream=0):
    return synth(po, n, d, stream=stream, r=16)


def _poison(la, floats):
    block = la.DeviceArray.from_host(np.full(floats, np.nan, np.float32))
    block.free()


@pytest.fixture(autouse=True)
def _recycled_memory(la, gpu):
    _poison(la, 4 * (N + 200) * 32)


def _widen(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def _check_f32_rows(la, s, X):
    """the handle's device rows [n x ld]: data columns = X bit for bit, padding columns +0.0"""
    gi = s.graph_info()
    n, d, ld = gi["n"], gi["dims"], gi["ld"]
    assert (n, d) == X.shape and ld == (d + 3) // 4 * 4
    raw = np.empty((n, ld), np.uint32)
    assert la.lib().leann_device_download(raw.ctypes.data, s.device_rows_ptr(), raw.nbytes) == 0
    assert (raw[:, :d] == np.ascontiguousarray(X).view(np.uint32)).all()
    assert (raw[:, d:] == 0).all()


def _check_bf16_rows(la, s, X):
    assert s.row_type() == la.RowType.BF16 and (s.export_rows_bf16() == la.round_bf16(X)).all()


def _check_search(po, s, X, Q, vamana=False, key_offset=0):
    """ids and distance bits of 16 queries = the oracle's walk of the exported graph over rows X"""
    g = s.graph_export()
    G = po.Graph.from_arrays(X, g["M"], g["M0"], g["max_level"], g["entry"], g["levels"], g["upper_off"], g["adj0"], g["adjU"])
    ok, od, oc, _ = G.search_batch(Q, K, EF, 1 if vamana else 0, 2)
    gk, gd, gc = s.search_batch(Q, K, EF)
    assert (gc == oc).all() and (gk == ok + np.uint64(key_offset)).all() and (gd.view(np.uint32) == od.view(np.uint32)).all()
    return gk, gd


def _oracle_arrays(po, X):
    G = po.Graph.build_hnsw(X, M=M, efc=EFC)
    return (M, 2 * M, G.max_level, G.entry) + tuple(G.export())


@pytest.mark.parametrize("d", DIMS)
def test_from_arrays(la, po, d):
    X, Q = _rows(po, N, d), _rows(po, 16, d, 1)
    s = la.BackendSearcher.from_arrays(la.BackendType.Hnsw, X, *_oracle_arrays(po, X))
    _check_f32_rows(la, s, X)
    _check_search(po, s, X, Q)
    s.close()


@pytest.mark.parametrize("d", DIMS)
def test_from_arrays_bf16_rows(la, po, d):
    X, Q = _rows(po, N, d), _rows(po, 16, d, 1)
    s = la.BackendSearcher.from_arrays(la.BackendType.Hnsw, X, *_oracle_arrays(po, X), row_type=la.RowType.BF16)
    _check_bf16_rows(la, s, X)
    _check_search(po, s, _widen(la.round_bf16(X)), Q)
    s.close()


@pytest.mark.parametrize("d", DIMS)
def test_build_to_a_file_and_load(la, po, tmp_path, d):
    X, Q = _rows(po, N, d), _rows(po, 16, d, 1)
    stem = str(tmp_path / "documents.leann")
    la.BackendBuilder(la.BackendType.Hnsw).build(X, [], stem, d, M, EFC)
    s = la.HnswSearcher.load(stem, d)
    _check_f32_rows(la, s, X)
    _check_search(po, s, X, Q)
    s.close()


@pytest.mark.parametrize("d", DIMS)
def test_build_bf16_rows_to_a_file_and_load(la, po, tmp_path, d):
    X, Q = _rows(po, N, d), _rows(po, 16, d, 1)
    stem = str(tmp_path / "documents.leann")
    la.BackendBuilder(la.BackendType.Hnsw).build(X, [], stem, d, M, EFC, row_type=la.RowType.BF16)
    s = la.HnswSearcher.load(stem, d)
    _check_bf16_rows(la, s, X)
    _check_search(po, s, _widen(la.round_bf16(X)), Q)
    s.close()


@pytest.mark.parametrize("d", DIMS)
def test_add_to_index_continues_the_build(la, po, tmp_path, d):
    X, Q = _rows(po, N + 200, d), _rows(po, 16, d, 1)
    stem = str(tmp_path / "documents.leann")
    B = la.BackendBuilder(la.BackendType.Hnsw)
    B.build(X[:N], [], stem, d, M, EFC)
    s = la.HnswSearcher.load(stem, d)
    before = s.graph_export()
    s.close()
    B.add_to_index(X[N:], stem, d, N)
    s = la.HnswSearcher.load(stem, d)
    _check_f32_rows(la, s, X)
    g = s.graph_export()
    assert (g["levels"][:N] == before["levels"]).all() and g["levels"][N:].any()  # the builder's levels, old and new
    _check_search(po, s, X, Q)
    s.close()


@pytest.mark.parametrize("d", DIMS)
def test_add_to_index_rebuilds_over_a_foreign_level_table(la, po, tmp_path, d):
    """a one-level graph (every level 0) is no table of the builder's: add_to_index rebuilds over old + new rows"""
    X, Q = _rows(po, N + 200, d), _rows(po, 16, d, 1)
    stem = str(tmp_path / "documents.leann")
    m, m0, _, entry, _, _, a0, _ = _oracle_arrays(po, X[:N])
    s = la.BackendSearcher.from_arrays(la.BackendType.Hnsw, X[:N], m, m0, 0, entry, np.zeros(N, np.uint8), np.zeros(N, np.uint32), a0,
                                       np.zeros((0, m), np.uint32))
    _check_search(po, s, X[:N], Q)
    s.save(stem)
    s.close()
    la.BackendBuilder(la.BackendType.Hnsw).add_to_index(X[N:], stem, d, N)
    s = la.HnswSearcher.load(stem, d)
    _check_f32_rows(la, s, X)
    g = s.graph_export()
    assert g["M"] == M and g["levels"][:N].any()  # rebuilt: the first N positions have the builder's levels now
    _check_search(po, s, X, Q)
    s.close()


@pytest.mark.parametrize("d", DIMS)
def test_append_host_rows(la, po, tmp_path, d):
    X, Q = _rows(po, N + 200, d), _rows(po, 16, d, 1)
    stem = str(tmp_path / "documents.leann")
    la.BackendBuilder(la.BackendType.Hnsw).build(X[:N], [], stem, d, M, EFC)
    s = la.HnswSearcher.load(stem, d)
    t = s.append(X[N:])
    _check_f32_rows(la, t, X)
    _check_search(po, t, X, Q)
    _check_f32_rows(la, s, X[:N])  # the source is as it was
    t.close()
    s.close()


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("backend", ["hnsw", "diskann"])
def test_stock_directory_rebuilt_from_the_embeddings(la, po, tmp_path, backend, d):
    stem, X, _ = _stock_dir(po, tmp_path / "idx", N, d, backend)
    kind = la.BackendType.from_name(backend)
    Q = _rows(po, 16, d, 1)
    s = la.BackendSearcher.load(kind, stem, d)
    _check_f32_rows(la, s, X)
    gk, gd = _check_search(po, s, X, Q, vamana=backend == "diskann")
    s.close()
    side = tmp_path / "idx" / ("documents.gpu.diskann" if backend == "diskann" else "documents.gpu.index")
    mtime = side.stat().st_mtime_ns
    s = la.BackendSearcher.load(kind, stem, d)  # second open: from the sidecar
    _check_f32_rows(la, s, X)
    k2, d2, _ = s.search_batch(Q, K, EF)
    assert (k2 == gk).all() and (d2.view(np.uint32) == gd.view(np.uint32)).all() and side.stat().st_mtime_ns == mtime
    s.close()


@pytest.mark.parametrize("d", DIMS)
def test_stock_directory_opened_in_two_shards(la, po, tmp_path, d):
    n = 700
    stem, X, _ = _stock_dir(po, tmp_path / "idx", n, d)
    Q = _rows(po, 16, d, 1)
    s = la.BackendSearcher.load(la.BackendType.Hnsw, stem, d, device="0,0")
    assert s.n_shards() == 2 and s.len() == n
    lo = 0
    for g in range(2):
        sh = s.shard(g)
        rows = X[lo:lo + sh.len()]
        assert (sh.graph_export(with_vectors=True)["vectors"] == rows).all()
        _check_f32_rows(la, sh, rows)
        _check_search(po, sh, rows, Q, key_offset=lo)
        lo += sh.len()
    assert lo == n
    first = s.search_batch(Q, K, EF)
    s.close()
    caches = [tmp_path / "idx" / f"documents.shard{g}of2.gpu.index" for g in range(2)]
    mtimes = [c.stat().st_mtime_ns for c in caches]
    s = la.BackendSearcher.load(la.BackendType.Hnsw, stem, d, device="0,0")  # second open: from the shard caches
    second = s.search_batch(Q, K, EF)
    assert all((a.view(np.uint32) == b.view(np.uint32)).all() for a, b in zip(first, second))
    assert [c.stat().st_mtime_ns for c in caches] == mtimes
    s.close()


@pytest.mark.parametrize("d", DIMS)
def test_rebuild_degree_from_the_environment(la, po, tmp_path, monkeypatch, d):
    """LEANN_REBUILD_DEGREE is read by the one rebuild both opens go through (at the call: no reload needed)"""
    monkeypatch.setenv("LEANN_REBUILD_DEGREE", "12")
    stem, X, _ = _stock_dir(po, tmp_path / "plain", N, d)
    s = la.BackendSearcher.load(la.BackendType.Hnsw, stem, d)
    assert s.graph_info()["M"] == 12 and s.graph_info()["M0"] == 24
    s.close()
    stem, X, _ = _stock_dir(po, tmp_path / "sharded", N, d)
    s = la.BackendSearcher.load(la.BackendType.Hnsw, stem, d, device="0,0")
    assert [s.shard(g).graph_info()["M"] for g in range(2)] == [12, 12]
    s.close()


def test_derived_handles_keep_their_parameters(la, gpu, monkeypatch):
    # the prune form, latched when the source is made, goes through append and compact: a repair on either result is one-stage
    D, R = 40, 8
    rng = np.random.default_rng(5)
    g = cr.random_graph(rng, "diskann", 40, D, R, R, 0)
    monkeypatch.setenv("LEANN_VAMANA_TWO_STAGE", "0")
    s = _searcher(la, g)
    monkeypatch.delenv("LEANN_VAMANA_TWO_STAGE")
    a = s.append((rng.integers(-2, 3, (20, D)) / 8.0).astype(np.float32))
    c, _ = a.compact()
    for r in (a, c):
        k = _graph_dict(r, "diskann")
        removed = rng.random(60) < 0.30
        removed[k["entry"]] = True
        want = cr.consolidate(k, removed, alpha=1.2, two_stage=False)
        assert (want["adj0"] != cr.consolidate(k, removed, alpha=1.2, two_stage=True)["adj0"]).any()  # the two forms differ here
        _round(r, k, removed, removed, want)
    for h in (c, a, s):
        h.close()
    # removals go through to_rows
    h = cr.random_graph(rng, "hnsw", 60, D, 8, 16, 2)
    s = _searcher(la, h)
    gone = np.array([3, 17, h["entry"]], np.uint64)
    assert s.remove(gone) == 3
    t = s.to_rows(la.RowType.BF16)
    assert t.row_type() == la.RowType.BF16 and t.len() == 60 and t.live_len() == s.live_len() == 57
    assert (t.removed_bitmap()[0] == s.removed_bitmap()[0]).all()
    keys, _, counts = t.search_batch(h["X"], 10, 60)  # every row as a query, the removed ones among them
    assert counts.all() and not np.isin(keys, gone).any()
    ks, _, cs = s.search_batch(h["X"], 10, 60)  # (these rows are bf16-exact: the bf16 index IS the f32 one)
    assert (keys == ks).all() and (counts == cs).all()
    t.close()
    s.close()
