"""-m gpu: every way into a filtered search gives the same answer.

A search can start from a host-pointer call (zero-copy through the pinned block for small batches, staged otherwise), from a
device-pointer call, under a per-call bitmap or a registered filter, on a plain handle or on a composite one, before a removal, with
repairs pending, and after leann_backend_consolidate.  All of them end in one routine (api.hip: leann_internal_search_plain), so two
calls that ask the same question on the same handle must agree bit for bit — keys, distance bit patterns and counts, ties included —
and no removed key may come back from any of them.  The refusals (a stride shorter than the bitmap, exact search without stored
vectors, a foreign registered filter) are checked through every entry point too.

Rows and queries have coordinates in {-2..2}/8 (tests/consolidate_ref.py), so distances are exact in f32."""
import ctypes as C

import numpy as np
import pytest

import consolidate_ref as cr
from util import SEED

pytestmark = pytest.mark.gpu

D, K, EF = 40, 10, 48
U64MAX = np.iinfo(np.uint64).max
INVALID, UNSUPPORTED = 1, 5


def _searcher(la, g, key_offset=0):
    return la.BackendSearcher.from_arrays(la.BackendType.Hnsw, g["X"], g["M"], g["M0"], g["max_level"], g["entry"], g["levels"],
                                          g["upper_off"], g["adj0"], g["adjU"], key_offset=key_offset)


def _handle(la, kind, rng):
    """(searcher, rows, entry points' positions): one 1536-row HNSW graph, or a composite of two (1024 + 768 rows)"""
    if kind == "plain":
        g = cr.random_graph(rng, "hnsw", 1536, D, 8, 16, 2)
        return _searcher(la, g), 1536, [g["entry"]]
    g0, g1 = cr.random_graph(rng, "hnsw", 1024, D, 8, 16, 1), cr.random_graph(rng, "hnsw", 768, D, 8, 16, 1)
    s = la.ShardedIndex.from_searchers([_searcher(la, g0), _searcher(la, g1, key_offset=1024)], take_ownership=True).as_backend()
    return s, 1792, [g0["entry"], 1024 + g1["entry"]]


def _device(la, s, Q, allow=None, exact=False):
    """a device-pointer call; allow: None, [nbytes] (shared) or [nq, stride] (one bitmap per query)"""
    nq = len(Q)
    dq, dk, dd, dc = la.DeviceArray.from_host(Q), la.DeviceArray((nq, K), np.uint64), la.DeviceArray((nq, K), np.float32), \
        la.DeviceArray(nq, np.uint32)
    da = la.DeviceArray.from_host(allow) if allow is not None else None
    stride = 0 if allow is None or allow.ndim == 1 else allow.shape[1]
    if exact:
        s.search_filtered_exact_batch_device(dq.ptr, nq, K, da.ptr, stride, dk.ptr, dd.ptr, dc.ptr)
    elif allow is not None:
        s.search_filtered_batch_device(dq.ptr, nq, K, EF, da.ptr, stride, dk.ptr, dd.ptr, dc.ptr)
    else:
        s.search_batch_device(dq.ptr, nq, K, EF, dk.ptr, dd.ptr, dc.ptr)
    la.sync()
    return dk.to_host(), dd.to_host(), dc.to_host()


def _same(got, want, what):
    assert (got[2] == want[2]).all(), f"{what}: counts differ"
    assert (got[0] == want[0]).all(), f"{what}: keys differ"
    assert (got[1].view(np.uint32) == want[1].view(np.uint32)).all(), f"{what}: distance bits differ"


def _only(res, ok, what):
    """every returned key is a position flagged in ok ([n] shared, or [nq, n]); the tail of each row is unused"""
    keys, _, counts = res
    for i in range(len(keys)):
        ids = keys[i, : counts[i]].astype(np.int64)
        assert (ok if ok.ndim == 1 else ok[i])[ids].all(), f"{what}: query {i} returned a removed / disallowed key"
        assert (keys[i, counts[i]:] == U64MAX).all(), what


@pytest.mark.parametrize("kind", ["plain", "composite"])
def test_every_entry_point_gives_the_same_answer(la, gpu, monkeypatch, kind):
    rng = np.random.default_rng(21 if kind == "plain" else 22)
    s, n, entries = _handle(la, kind, rng)
    nbytes = (n + 7) // 8
    stride = (nbytes + 15) & ~15
    Q24 = (rng.integers(-2, 3, (24, D)) / 8.0).astype(np.float32)
    removed = np.zeros(n, bool)
    for state in ("no removals", "repairs pending", "consolidated"):
        if state == "repairs pending":
            removed = rng.random(n) < 0.25
            removed[entries] = True                              # the entry points go too
            keys = np.flatnonzero(removed).astype(np.uint64)
            assert s.remove(keys) == len(keys) and s.removed_bitmap()[1] > 0
        if state == "consolidated":
            s.consolidate()
            assert s.removed_bitmap()[1] == 0
        live = ~removed
        allowed = rng.random(n) < 0.5
        allowed[np.flatnonzero(removed)[:50]] = True             # the caller's bitmaps allow removed positions
        shared = np.packbits(allowed, bitorder="little")
        allowed_q = rng.random((24, n)) < 0.5
        allowed_q[:, np.flatnonzero(removed)[:50]] = True
        per_query = np.zeros((24, stride), np.uint8)
        per_query[:, :nbytes] = np.packbits(allowed_q, axis=1, bitorder="little")
        flt = s.register_filter(shared)                          # (a filter predating a removal is refused: one per state)
        assert flt.count() == int((allowed & live).sum()) < 65536
        for nq in (3, 24):                                       # 3: queries read in place from the pinned block; 24: one DMA of them
            Q, pq, aq = Q24[:nq], per_query[:nq], allowed_q[:nq]
            what = f"{kind}, {state}, nq={nq}"
            dev_walk, dev_shared, dev_pq = _device(la, s, Q), _device(la, s, Q, shared), _device(la, s, Q, pq)
            dev_exact = _device(la, s, Q, shared, exact=True)
            _only(dev_walk, live, what)
            _only(dev_shared, live & allowed, what)
            _only(dev_pq, live[None, :] & aq, what)
            _only(dev_exact, live & allowed, what)
            assert (dev_walk[2] > 0).all() and (dev_exact[2] == K).all()
            for staged in (False, True):                         # the host path: zero-copy, then staged through device buffers
                if staged:
                    monkeypatch.setenv("LEANN_DEBUG_NO_ZERO_COPY", "1")
                else:
                    monkeypatch.delenv("LEANN_DEBUG_NO_ZERO_COPY", raising=False)
                la.lib().leann_debug_reload_env()
                w = f"{what}, {'staged' if staged else 'zero-copy'}"
                _same(s.search_batch(Q, K, EF), dev_walk, w + ": unfiltered walk, host against device")
                _same(s.search_filtered_batch(Q, K, EF, shared), dev_shared, w + ": walk under a shared bitmap, host against device")
                _same(s.search_filtered_batch(Q, K, EF, pq), dev_pq, w + ": walk under per-query bitmaps, host against device")
                _same(s.search_filtered_exact_batch(Q, K, shared), dev_exact, w + ": exact under a shared bitmap, host against device")
                _same(s.search_filter_batch(Q, K, EF, flt, "walk"), dev_shared, w + ": registered filter, walk")
                _same(s.search_filter_batch(Q, K, EF, flt, "exact"), dev_exact, w + ": registered filter, exact")
                # auto: exact, since the filter allows fewer than 65536 rows and nq <= 64 (api.hip, FILTER_AUTO)
                _same(s.search_filter_batch(Q, K, EF, flt, "auto"), dev_exact, w + ": registered filter, auto")
        flt.close()
    monkeypatch.delenv("LEANN_DEBUG_NO_ZERO_COPY", raising=False)
    la.lib().leann_debug_reload_env()
    s.close()


def _raw_calls(la, s, Q, allow, stride, exact_only=False):
    """every entry point that takes a bitmap, straight through the C ABI (the Python wrappers check shapes themselves):
    yields (name, return code, message)"""
    L = la.lib()
    f32p, u64p, u32p, u8p = (C.POINTER(t) for t in (C.c_float, C.c_uint64, C.c_uint32, C.c_uint8))
    nq = len(Q)
    keys, dists, counts = np.zeros((nq, K), np.uint64), np.zeros((nq, K), np.float32), np.zeros(nq, np.uint32)
    out = (keys.ctypes.data_as(u64p), dists.ctypes.data_as(f32p), counts.ctypes.data_as(u32p))
    q, a = Q.ctypes.data_as(f32p), allow.ctypes.data_as(u8p)
    dq, da = la.DeviceArray.from_host(Q), la.DeviceArray.from_host(allow)
    dk, dd, dc = la.DeviceArray((nq, K), np.uint64), la.DeviceArray((nq, K), np.float32), la.DeviceArray(nq, np.uint32)
    calls = [("exact, host", lambda: L.leann_backend_search_filtered_exact_batch(s._h, q, nq, K, a, stride, *out)),
             ("exact, device", lambda: L.leann_backend_search_filtered_exact_batch_device(s._h, dq.ptr, nq, K, da.ptr, stride, dk.ptr, dd.ptr,
                                                                                          dc.ptr, None))]
    if not exact_only:
        calls += [("walk, host", lambda: L.leann_backend_search_filtered_batch(s._h, q, nq, K, EF, a, stride, *out)),
                  ("walk, device", lambda: L.leann_backend_search_filtered_batch_device(s._h, dq.ptr, nq, K, EF, da.ptr, stride, dk.ptr,
                                                                                        dd.ptr, dc.ptr, None, None))]
    for name, call in calls:
        rc = call()
        yield name, rc, L.leann_last_error().decode("utf-8", "replace")
    la.sync()


@pytest.mark.parametrize("kind", ["plain", "composite"])
def test_short_stride_and_foreign_filter_are_refused(la, gpu, kind):
    rng = np.random.default_rng(23)
    s, n, _ = _handle(la, kind, rng)
    other, n_other, _ = _handle(la, "composite" if kind == "plain" else "plain", rng)
    nbytes = (n + 7) // 8
    Q = (rng.integers(-2, 3, (4, D)) / 8.0).astype(np.float32)
    allow = np.full((4, nbytes), 0xFF, np.uint8)
    for name, rc, msg in _raw_calls(la, s, Q, allow, nbytes - 1):   # per-query bitmaps one byte too close together
        assert rc == INVALID and "allow_stride" in msg, (kind, name, rc, msg)
    for name, rc, msg in _raw_calls(la, s, Q, allow, nbytes):       # (the same calls with the right stride go through)
        assert rc == 0, (kind, name, rc, msg)
    flt = other.register_filter(np.full((n_other + 7) // 8, 0xFF, np.uint8))
    for mode in ("walk", "exact", "auto"):
        with pytest.raises(la.LeannError) as e:
            s.search_filter_batch(Q, K, EF, flt, mode)
        assert e.value.code == INVALID, (kind, mode)
    flt.close()
    other.close()
    s.close()


def test_exact_search_without_stored_vectors_is_refused(la, po, gpu):
    """the recompute-on graph of tests/test_gpu_filtered.py::test_filtered_recompute_on_graph, alone and as a one-shard composite"""
    n, h, d, M = 6000, 256, 768, 16
    rng = np.random.default_rng(24)
    Lc, chk = la.lib(), la._native.check
    dF, dW = la.DeviceArray.from_host(po.synth_features(SEED, h, 64, 1.0, 0, 0, n)), la.DeviceArray.from_host(po.synth_weights(SEED, h, d))
    r, hb = C.c_void_p(), C.c_void_p()
    chk(Lc.leann_recompute_create(dF.ptr, n, h, dW.ptr, d, 0, 0, C.byref(r)))
    chk(Lc.leann_recompute_build_index(r, 0, M, 64, C.byref(hb)))
    plain = la.BackendSearcher(hb, la.BackendType.Hnsw)
    composite = la.ShardedIndex.from_searchers([plain], take_ownership=False).as_backend()
    Q = rng.standard_normal((4, d)).astype(np.float32)
    allow = np.full((4, (n + 7) // 8), 0xFF, np.uint8)
    for kind, s in (("plain", plain), ("composite", composite)):
        for stride in (0, allow.shape[1]):
            for name, rc, msg in _raw_calls(la, s, Q, allow, stride, exact_only=True):
                assert rc == UNSUPPORTED and "exact filtered search needs stored vectors" in msg, (kind, name, stride, rc, msg)
        flt = s.register_filter(allow[0])
        with pytest.raises(la.LeannError) as e:
            s.search_filter_batch(Q, K, EF, flt, "exact")
        assert e.value.code == UNSUPPORTED and "exact filtered search needs stored vectors" in str(e.value), kind
        flt.close()
    composite.close()
    plain.close()
    Lc.leann_recompute_close(r)
