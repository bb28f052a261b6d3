"""-m gpu: buffers that are grown on demand and kept give the answers of buffers made for the call.

The host-pointer search keeps a workspace per concurrent caller (api.hip: Workspace — d_q, d_keys, d_dists, d_counts, d_stats and the
pinned block), a handle with removals keeps one AND-ed bitmap per stream (consolidate.hip: live_scratch) and a recompute-on handle one
block of projected queries per stream (api.hip: proj_scratch).  Each grows to the largest request it has seen and is then reused by
smaller ones.  Here ONE handle, from one thread, sees a small call, a larger one, one that outgrows every buffer, and a small one
again; every answer must equal — keys, f32 distance bits and counts — the same call on a freshly opened handle of the same index,
whose buffers were made for exactly that call, and for the unfiltered calls the oracle's walk of the same graph as well.

One index: n = 2000, d = 64, HNSW degree 8, k = 10.  Host-pointer search_batch with nq = 1 (zero-copy, queries read in place from the
pinned block), 70 (zero-copy, queries copied to d_q), NQ_STAGED (the layout of search_filtered_batch_host_impl no longer fits the
256 KiB pinned block: staged, all five buffers grown) and 3 (buffers larger than needed).  After removing 5 rows: the filtered device
entry point under per-query bitmaps with nq = 5 and then 40, queued on one caller stream, so the stream's live_scratch is replaced
between two queued calls.  A recompute-on index of the same size (feat_h 64): nq = 2 and then 50 queued on one stream, so its
proj_scratch is."""
import ctypes as C

import numpy as np
import pytest

from util import SEED, HipStreams, synth

pytestmark = pytest.mark.gpu

N, D, M, K, EF = 2000, 64, 8, 10, 64
U64MAX = np.iinfo(np.uint64).max


def _pin_bytes(nq, d=D, k=K):
    """the pinned block a host-pointer call of nq queries needs (api.hip, search_filtered_batch_host_impl: 16-byte aligned pieces
    {queries | keys | dists | counts | stats})"""
    a16 = lambda x: (x + 15) & ~15
    o_keys = a16(nq * d * 4)
    o_dists = o_keys + nq * k * 8
    o_counts = a16(o_dists + nq * k * 4)
    o_stats = o_counts + a16(nq * 4)
    return o_stats + nq * 16


NQ_STAGED = next(nq for nq in range(1, 4096) if _pin_bytes(nq) > (256 << 10))  # the first batch that is staged: 662


@pytest.fixture(scope="module")
def index(po):
    X = synth(po, N, D)
    G = po.Graph.build_hnsw(X, M=M, efc=64)
    Q = synth(po, NQ_STAGED, D, stream=1)
    return X, G, G.export(), Q


def _open(la, index):
    X, G, (lv, uo, a0, aU), _ = index
    return la.BackendSearcher.from_arrays(la.BackendType.Hnsw, X, M, 2 * M, G.max_level, G.entry, lv, uo, a0, aU)


def _same(got, want, what):
    assert (got[2] == want[2]).all(), f"{what}: counts differ"
    assert (got[0] == want[0]).all(), f"{what}: keys differ in {(got[0] != want[0]).any(axis=1).sum()} queries"
    assert (got[1].view(np.uint32) == want[1].view(np.uint32)).all(), f"{what}: distance bits differ"


def test_workspace_of_the_host_pointer_search_regrows(la, po, gpu, index):
    _, G, _, Qall = index
    s = _open(la, index)
    for nq in (1, 70, NQ_STAGED, 3):
        Q = Qall[:nq]
        got = s.search_batch(Q, K, EF)
        fresh = _open(la, index)
        _same(got, fresh.search_batch(Q, K, EF), f"nq = {nq}, against a fresh handle")
        fresh.close()
        ok, od, oc, _ = G.search_batch(Q, K, EF, 0, nthreads=8)
        _same(got, (ok, od, oc), f"nq = {nq}, against the oracle")
    s.close()


def _queued(la, s, calls, stream):
    """the device calls of `calls` [(queries, bitmaps or None)] queued on `stream` with nothing in between, then one synchronisation"""
    held, outs = [], []
    for Q, allow in calls:
        nq = len(Q)
        dq, dk, dd, dc = la.DeviceArray.from_host(Q), la.DeviceArray.from_host(np.full((nq, K), U64MAX, np.uint64)), \
            la.DeviceArray((nq, K), np.float32), la.DeviceArray(nq, np.uint32)
        da = la.DeviceArray.from_host(allow) if allow is not None else None
        held.append((dq, da))
        outs.append((dk, dd, dc))
    la.sync()  # the uploads and prefills above are null-stream work
    for (dq, da), (dk, dd, dc), (Q, allow) in zip(held, outs, calls):
        if allow is None:
            s.search_batch_device(dq.ptr, len(Q), K, EF, dk.ptr, dd.ptr, dc.ptr, stream=stream)
        else:
            s.search_filtered_batch_device(dq.ptr, len(Q), K, EF, da.ptr, allow.shape[1], dk.ptr, dd.ptr, dc.ptr, stream=stream)
    la.sync()
    return [(dk.to_host(), dd.to_host(), dc.to_host()) for dk, dd, dc in outs]


def test_live_scratch_of_a_stream_regrows(la, gpu, index):
    _, _, _, Qall = index
    rng = np.random.default_rng(7)
    removed = rng.choice(N, 5, replace=False).astype(np.uint64)
    nbytes = (N + 7) // 8
    stride = (nbytes + 15) & ~15
    calls = []
    for nq in (5, 40):
        allowed = rng.random((nq, N)) < 0.5
        allowed[:, removed.astype(np.int64)] = True  # the caller allows the removed rows; the live mask must not
        bitmaps = np.zeros((nq, stride), np.uint8)
        bitmaps[:, :nbytes] = np.packbits(allowed, axis=1, bitorder="little")
        calls.append((Qall[100:100 + nq], bitmaps))
    s = _open(la, index)
    assert s.remove(removed) == 5
    with HipStreams(la, 1) as sts:
        got = _queued(la, s, calls, sts[0])
        for call, g in zip(calls, got):
            fresh = _open(la, index)
            assert fresh.remove(removed) == 5
            _same(g, _queued(la, fresh, [call], sts[0])[0], f"nq = {len(call[0])}, per-query bitmaps, against a fresh handle")
            fresh.close()
            assert (g[2] > 0).all() and not np.isin(g[0], removed).any()
    s.close()


def test_proj_scratch_of_a_stream_regrows(la, po, gpu, tmp_path):
    h = 64
    Lc, chk = la.lib(), la._native.check
    F = po.synth_features(SEED, h, 64, 1.0, 0, 0, N)
    W = po.synth_weights(SEED, h, D)
    Q = po.recompute_encode(po.synth_features(SEED, h, 64, 1.0, 1, 0, 50), W)
    dF, dW = la.DeviceArray.from_host(F), la.DeviceArray.from_host(W)
    r, hb = C.c_void_p(), C.c_void_p()
    chk(Lc.leann_recompute_create(dF.ptr, N, h, dW.ptr, D, 0, 0, C.byref(r)))
    chk(Lc.leann_recompute_build_index(r, 0, M, 64, C.byref(hb)))
    s = la.BackendSearcher(hb, la.BackendType.Hnsw)
    stem = str(tmp_path / "documents.leann")
    s.save(stem)
    calls = [(Q[:2], None), (Q, None)]
    with HipStreams(la, 1) as sts:
        got = _queued(la, s, calls, sts[0])
        for call, g in zip(calls, got):
            fresh = la.BackendSearcher.load(la.BackendType.Hnsw, stem, D)
            _same(g, _queued(la, fresh, [call], sts[0])[0], f"recompute-on graph, nq = {len(call[0])}, against a freshly opened handle")
            fresh.close()
            assert (g[2] == K).all()
    s.close()
    Lc.leann_recompute_close(r)
