"""-m gpu: whatever the library allocates on the device for a handle, a filter or a call is given back when that is closed or returns.

leann_debug_device_blocks() counts the device blocks the library owns at this moment: every DeviceBuf (csrc/device_mem.h) and every
lease of the scratch pool; blocks resting in the pool and the caller's own leann_device_malloc memory (DeviceArray) do not count.
Each test takes the count c0, makes things, sees the count rise, closes them and sees c0 again — so a member that close forgets, a
lease that an early return keeps, or a borrowed row array that close frees by mistake (the caller's array is read back afterwards)
shows here, on a shared card, where device-wide free memory says nothing.

Index shape unless said otherwise: n = 2000, d = 64, HNSW degree 8, k = 10, ef = 64 (as tests/test_gpu_scratch_regrow.py)."""
import ctypes as C
import gc

import numpy as np
import pytest

from test_gpu_scratch_regrow import NQ_STAGED
from util import SEED, HipStreams, synth

pytestmark = pytest.mark.gpu

N, D, M, K, EF = 2000, 64, 8, 10, 64
U64MAX = np.iinfo(np.uint64).max
INVALID = 1  # LEANN_ERR_INVALID


def _blocks(la):
    gc.collect()  # a searcher an earlier test dropped without close() must not be closed by the collector half way through this one
    return int(la.lib().leann_debug_device_blocks())


@pytest.fixture(scope="module")
def index(po):
    X = synth(po, N, D)
    G = po.Graph.build_hnsw(X, M=M, efc=64)
    Q = synth(po, NQ_STAGED, D, stream=1)
    return X, G, G.export(), Q


def _open(la, index, **kw):
    X, G, (lv, uo, a0, aU), _ = index
    return la.BackendSearcher.from_arrays(la.BackendType.Hnsw, X, M, 2 * M, G.max_level, G.entry, lv, uo, a0, aU, **kw)


def _device_search(la, s, Q, allow=None, stream=None, k=K):
    """one device call (per-query bitmaps `allow` [nq x stride] or none) and its answer on the host"""
    nq = len(Q)
    dq, dk = la.DeviceArray.from_host(Q), la.DeviceArray.from_host(np.full((nq, k), U64MAX, np.uint64))
    dd, dc = la.DeviceArray((nq, k), np.float32), la.DeviceArray(nq, np.uint32)
    da = la.DeviceArray.from_host(allow) if allow is not None else None
    la.sync()
    if allow is None:
        s.search_batch_device(dq.ptr, nq, k, EF, dk.ptr, dd.ptr, dc.ptr, stream=stream)
    else:
        s.search_filtered_batch_device(dq.ptr, nq, k, EF, da.ptr, allow.shape[1], dk.ptr, dd.ptr, dc.ptr, stream=stream)
    la.sync()
    return dk.to_host(), dd.to_host(), dc.to_host()


def _same(got, want, what):
    assert (got[2] == want[2]).all(), f"{what}: counts differ"
    assert (got[0] == want[0]).all(), f"{what}: keys differ"
    assert (got[1].view(np.uint32) == want[1].view(np.uint32)).all(), f"{what}: distance bits differ"


def test_from_arrays_handle_with_both_visited_pools(la, gpu, index, monkeypatch):
    monkeypatch.setenv("LEANN_DEBUG_GPOOL_BITS", "6")  # 64-slot tables cannot hold n + 128 positions: the second pool is made too
    la.lib().leann_debug_reload_env()
    c0 = _blocks(la)
    s = _open(la, index)
    c_open = _blocks(la)
    assert c_open >= c0 + 5, "rows, three graph arrays and the level table"
    for nq in (1, 70, NQ_STAGED):  # zero-copy in place, zero-copy with copied queries, the first staged batch
        _, _, counts = s.search_batch(index[3][:nq], K, EF)
        assert (counts == K).all()
    assert _blocks(la) >= c_open + 4 + 5, "two pools with their locks, and the staged workspace"
    s.close()
    assert _blocks(la) == c0


def test_build_device_borrows_or_copies_the_rows(la, gpu, index):
    X, _, _, Qall = index
    Q = Qall[:20]
    c0 = _blocks(la)
    dX = la.DeviceArray.from_host(X)
    s = la.BackendSearcher.build_device(la.BackendType.Hnsw, dX.ptr, N, D, D, M, 64)
    assert _blocks(la) > c0
    borrowed = _device_search(la, s, Q)
    assert (borrowed[2] == K).all()
    s.close()
    assert _blocks(la) == c0
    assert (dX.to_host().view(np.uint32) == X.view(np.uint32)).all(), "close must leave borrowed rows alone"
    dX.free()

    dX = la.DeviceArray.from_host(X)
    s = la.BackendSearcher.build_device(la.BackendType.Hnsw, dX.ptr, N, D, D, M, 64, take_copy=True)
    dX.free()  # the handle searches its own copy
    assert _blocks(la) > c0
    _same(_device_search(la, s, Q), borrowed, "take_copy handle against the borrowed one")
    s.close()
    assert _blocks(la) == c0


def test_bf16_row_stores(la, gpu, index):
    X, _, _, Qall = index
    c0 = _blocks(la)
    dX = la.DeviceArray.from_host(X)
    built = la.BackendSearcher.build_device(la.BackendType.Hnsw, dX.ptr, N, D, D, M, 64, row_type=la.RowType.BF16, may_overwrite=False)
    c_built = _blocks(la)
    assert c_built > c0
    assert (dX.to_host().view(np.uint32) == X.view(np.uint32)).all(), "may_overwrite=False: the caller's rows stay as they are"
    dX.free()
    from_arrays = _open(la, index, row_type=la.RowType.BF16)
    c_two = _blocks(la)
    assert c_two > c_built
    f32 = _open(la, index)
    converted = f32.to_rows(la.RowType.BF16)
    assert _blocks(la) > c_two
    for s in (built, from_arrays, converted):
        assert s.row_type() == la.RowType.BF16
        assert (s.search_batch(Qall[:8], K, EF)[2] == K).all()
    _same(converted.search_batch(Qall[:8], K, EF), from_arrays.search_batch(Qall[:8], K, EF), "to_rows against from_arrays(BF16)")
    for s in (converted, f32, from_arrays, built):
        s.close()
    assert _blocks(la) == c0


def test_row_screen_planes(la, po, gpu):
    n, d = 300, 520  # three 256-float chunks per row
    X = synth(po, n, d)
    G = po.Graph.build_hnsw(X, M=M, efc=64)
    lv, uo, a0, aU = G.export()
    c0 = _blocks(la)
    s = la.BackendSearcher.from_arrays(la.BackendType.Hnsw, X, M, 2 * M, G.max_level, G.entry, lv, uo, a0, aU)
    c_open = _blocks(la)
    s.set_row_screen(True)
    assert _blocks(la) == c_open + 3, "two planes and the counters"
    assert (s.search_batch(synth(po, 64, d, stream=1), K, EF)[2] == K).all()
    s.close()
    assert _blocks(la) == c0


def test_removals_live_mask_and_consolidate(la, gpu, index):
    _, _, _, Qall = index
    rng = np.random.default_rng(7)
    removed = rng.choice(N, 5, replace=False).astype(np.uint64)
    nbytes = (N + 7) // 8
    stride = (nbytes + 15) & ~15
    c0 = _blocks(la)
    s = _open(la, index)
    c_open = _blocks(la)
    assert s.remove(removed) == 5
    assert _blocks(la) == c_open + 1, "the live mask"
    with HipStreams(la, 1) as sts:
        for nq in (5, 40):  # the stream's AND-ed bitmap block is made, then replaced by a larger one
            allowed = rng.random((nq, N)) < 0.5
            bitmaps = np.zeros((nq, stride), np.uint8)
            bitmaps[:, :nbytes] = np.packbits(allowed, axis=1, bitorder="little")
            keys, _, counts = _device_search(la, s, Qall[:nq], allow=bitmaps, stream=sts[0])
            assert (counts > 0).all() and not np.isin(keys, removed).any()
    assert _blocks(la) > c_open + 1
    s.consolidate()
    assert s.removed_bitmap()[1] == 0
    s.close()
    assert _blocks(la) == c0


def _filter_round(la, s, Q, allow, c_handle):
    f = s.register_filter(allow)
    assert _blocks(la) > c_handle
    exact = s.search_filter_batch(Q, K, EF, f, mode="exact")
    walk = s.search_filter_batch(Q, K, EF, f, mode="walk")
    assert (exact[2] == K).all() and (walk[2] > 0).all()
    f.close()


def test_registered_filter_on_a_plain_and_a_composite_handle(la, gpu, index):
    X, _, _, Qall = index
    allow = np.packbits(np.random.default_rng(3).random(N) < 0.3, bitorder="little")
    c0 = _blocks(la)
    s = _open(la, index)
    s.search_batch(Qall[:4], K, EF)  # pools and workspace exist before the level is taken
    _filter_round(la, s, Qall[:4], allow, _blocks(la))  # (its searches may grow the workspace: the level is taken again below)
    c_handle = _blocks(la)
    _filter_round(la, s, Qall[:4], allow, c_handle)
    assert _blocks(la) == c_handle, "Filter.close() gives back the bitmap and the list, nothing else moved"
    s.close()
    assert _blocks(la) == c0

    lows = [0, 960, N]  # interior boundaries are multiples of 64
    parts = [la.DeviceArray.from_host(X[lows[g]:lows[g + 1]]) for g in range(2)]
    comp = la.ShardedIndex.build_device(la.BackendType.Hnsw, [p.ptr for p in parts], [lows[g + 1] - lows[g] for g in range(2)], D, D, M, 64,
                                        [0, 0], keep=parts).as_backend()
    comp.search_batch(Qall[:4], K, EF)
    _filter_round(la, comp, Qall[:4], allow, _blocks(la))
    c_handle = _blocks(la)
    _filter_round(la, comp, Qall[:4], allow, c_handle)
    assert _blocks(la) == c_handle
    comp.close()
    assert _blocks(la) == c0


@pytest.mark.parametrize("h,d", [(64, 64), (256, 384)])  # inline norm; split layout with the norms in an array of their own
def test_recompute_on_index_built_saved_and_loaded(la, po, gpu, tmp_path, h, d):
    Lc, chk = la.lib(), la._native.check
    F = po.synth_features(SEED, h, 64, 1.0, 0, 0, N)
    W = po.synth_weights(SEED, h, d)
    Q = po.recompute_encode(po.synth_features(SEED, h, 64, 1.0, 1, 0, 6), W)
    dF, dW = la.DeviceArray.from_host(F), la.DeviceArray.from_host(W)
    c0 = _blocks(la)
    r, hb = C.c_void_p(), C.c_void_p()
    chk(Lc.leann_recompute_create(dF.ptr, N, h, dW.ptr, d, 0, 0, C.byref(r)))
    c_r = _blocks(la)
    chk(Lc.leann_recompute_build_index(r, 0, M, 64, C.byref(hb)))
    built = la.BackendSearcher(hb, la.BackendType.Hnsw)
    c_built = _blocks(la)
    assert c_built >= c_r + 6 + (h == 256), "feature rows, weights, graph arrays (and the norms); the embeddings are gone"
    stem = str(tmp_path / "documents.leann")
    built.save(stem)
    loaded = la.BackendSearcher.load(la.BackendType.Hnsw, stem, d)
    assert _blocks(la) >= c_built + 6 + (h == 256), "the same arrays again (the built handle also has the pools its build searched with)"
    got = _device_search(la, built, Q)
    assert (got[2] == K).all()
    _same(_device_search(la, loaded, Q), got, "loaded recompute-on index against the built one")
    loaded.close()
    built.close()
    assert _blocks(la) == c_r
    Lc.leann_recompute_close(r)
    assert _blocks(la) == c0


def test_composite_handle_with_staging_buffers(la, gpu, index, tmp_path, monkeypatch):
    X, _, _, Qall = index
    monkeypatch.setenv("LEANN_DEBUG_FORCE_REMOTE", "1")  # every shard is treated as remote: staging buffers and peer copies
    la.lib().leann_debug_reload_env()
    lows = [0, 960, N]
    parts = [la.DeviceArray.from_host(X[lows[g]:lows[g + 1]]) for g in range(2)]
    c0 = _blocks(la)
    comp = la.ShardedIndex.build_device(la.BackendType.Hnsw, [p.ptr for p in parts], [lows[g + 1] - lows[g] for g in range(2)], D, D, M, 64,
                                        [0, 0], keep=parts).as_backend()
    c_built = _blocks(la)
    assert c_built > c0
    got = _device_search(la, comp, Qall[:30])
    assert (got[2] == K).all() and got[0].max() >= lows[1]
    assert _blocks(la) > c_built, "the staging buffers of the remote branch"
    stem = str(tmp_path / "documents.leann")
    comp.save(stem)
    again = la.BackendSearcher.load(la.BackendType.Hnsw, stem, D, device="0,0")
    assert again.n_shards() == 2
    _same(_device_search(la, again, Qall[:30]), got, "reopened composite against the built one")
    again.close()
    comp.close()
    assert _blocks(la) == c0


@pytest.mark.parametrize("n", [2000, 70_000])  # one slab; above the 64k-row threshold: candidate emission, all five scratch blocks
def test_exact_scan_returns_its_scratch(la, po, gpu, n):
    nq, k = 3, 10
    X = synth(po, n, D)
    Q = synth(po, nq, D, stream=1)
    dX, dQ = la.DeviceArray.from_host(X), la.DeviceArray.from_host(Q)
    dk, ds, dc = la.DeviceArray((nq, k), np.uint64), la.DeviceArray((nq, k), np.float32), la.DeviceArray(nq, np.uint32)
    c0 = _blocks(la)
    for _ in range(2):  # the second call finds the first one's blocks in the pool
        la._native.check(la.lib().leann_scan_topk_device(dX.ptr, n, D, D, dQ.ptr, nq, k, None, 0, dk.ptr, ds.ptr, dc.ptr, None))
        assert _blocks(la) == c0
    keys, scores = dk.to_host(), ds.to_host()
    assert (dc.to_host() == k).all()
    S = X.astype(np.float64) @ Q.astype(np.float64).T
    assert np.allclose(scores[:, 0], S.max(axis=0), rtol=0, atol=1e-4) and (np.abs(S[keys[:, 0], np.arange(nq)] - S.max(axis=0)) < 1e-4).all()


def test_bm25_handle(la, gpu):
    words = "rust python kernel graph vector search index query gpu wave lds bank memory cache".split()
    rng = np.random.default_rng(3)
    docs = [" ".join(rng.choice(words, size=int(rng.integers(2, 25)))) for _ in range(400)] + ["", "a b c"]
    c0 = _blocks(la)
    idx = la.Bm25Index.from_texts(docs)
    assert _blocks(la) > c0
    _, _, cnt, _, _ = idx.search_batch(["rust rust kernel", "", "gpu wave lds bank memory cache gpu"], 3)
    assert list(cnt) == [3, 0, 3]
    idx.close()
    assert _blocks(la) == c0


def test_error_returns_after_allocation_leave_nothing(la, gpu, index, tmp_path):
    X = index[0]
    stem = str(tmp_path / "documents.leann")
    s = _open(la, index)
    s.save(stem)
    s.close()
    c0 = _blocks(la)
    # appended ids must continue the index: refused after the index is open on the device
    with pytest.raises(la.LeannError) as e:
        la.BackendBuilder(la.BackendType.Hnsw).add_to_index(X[:4], stem, D, N + 1)
    assert e.value.code == INVALID and "does not continue" in str(e.value)
    assert _blocks(la) == c0
    # half a file: a short read on the host
    path = tmp_path / "documents.index"
    raw = path.read_bytes()
    path.write_bytes(raw[: len(raw) // 2])
    with pytest.raises(la.LeannError):
        la.BackendSearcher.load(la.BackendType.Hnsw, stem, D)
    assert _blocks(la) == c0
