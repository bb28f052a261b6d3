"""-m gpu: the *_device entry points on caller streams, with other calls in flight on the same handle (they take a
hipStream_t, never synchronise and, once warm, allocate nothing).  Every other GPU test passes the null stream and synchronises
before it looks, where a piece of a search queued on the wrong stream, a scratch buffer shared by two calls in flight or a slot reused
too early cannot change an answer.  Bar of every leg: the same call on a non-blocking stream, overlapped with others, returns the
bytes the call returns on the null stream — keys, f32 distance bits, counts and the [nq x 4] stats rows.  No tolerances, no timing
assertion (wall times are printed for the log only).

Shape of a leg (_serial / _overlapped): the serial answer of every query set (null stream, then la.sync()); the same calls on S
non-blocking streams, round-robin, several rounds, no host synchronisation in between, every stream with output and stats buffers of
its own and the set it gets rotating from round to round (stale bytes of an earlier round cannot match); one la.sync(); the last
round's buffers against the serial answers.

    leg                                       shared state held
    1  plain f32 HNSW handle                  launch path of api.hip on a caller stream (+ queries produced on that stream, + the
                                              rerank of hybrid.hip queued behind the search)
    2  tiny visited tables                    the visited-set pools, their device-side locks and the generation counter
                                              (hop_migrate.cuh, ensure_gpool), across launches
    3  removals + caller bitmaps              live_scratch[stream] (consolidate.hip: leann_internal_live_allow)
    4  recompute-on graph handles             proj_scratch[stream] (api.hip: project_queries), h = 256 and h = 100
    5  row screen                             screen_ctr, the device atomics every launch of a handle adds to
    6  bf16 rows                              launch path of search_bf16.hip on a caller stream
    7  synchronous calls from threads         the process-wide scratch pool of scan.hip, blocks changing hands between threads
    8  composite handle                       the two rotating result slots, their event chain and the per-shard staging buffers
                                              (shard.hip), synchronous and ticket form, local and forced-remote branch
    9  HIP-graph replay (child process)       capturability: fork -> 8 calls on 8 streams -> join, replayed over changing queries
"""
import ctypes as C
import itertools
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

from util import SEED, HipStreams, synth

pytestmark = pytest.mark.gpu
K, EF = 10, 64


# ---- the shape of every leg -------------------------------------------------------------------------------------------------------------
class _Out:
    """one call's outputs in HBM — keys, distances (scores), counts and, if asked for, the stats rows —, prefilled with a pattern no
    answer holds"""

    def __init__(self, la, nq, k, stats=True):
        self.keys = la.DeviceArray.from_host(np.full((nq, k), 0xABABABABABABABAB, np.uint64))
        self.dists = la.DeviceArray.from_host(np.full((nq, k), 0xABABABAB, np.uint32).view(np.float32))
        self.counts = la.DeviceArray.from_host(np.full(nq, 0xABABABAB, np.uint32))
        self.stats = la.DeviceArray.from_host(np.full((nq, 4), 0xABABABAB, np.uint32)) if stats else None

    def ptrs(self):
        return self.keys.ptr, self.dists.ptr, self.counts.ptr

    def poison(self):
        """the keys back to the pattern, so that an answer left by an earlier call cannot pass for this one's (blocks until done)"""
        self.keys.upload(np.full(self.keys.shape, 0xABABABABABABABAB, np.uint64))

    def host(self):
        """(keys, distance bits, counts[, stats]) — call after a synchronisation"""
        r = (self.keys.to_host(), self.dists.to_host().view(np.uint32), self.counts.to_host())
        return r + (self.stats.to_host(),) if self.stats is not None else r


NAMES = ("keys", "distance bits", "counts", "stats")


def _assert_same(got, want, what):
    assert len(got) == len(want)
    for name, a, b in zip(NAMES, got, want):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name)
        if a.tobytes() != b.tobytes():
            rows = (a.reshape(len(a), -1) != b.reshape(len(b), -1)).any(axis=1)
            raise AssertionError(f"{what}: {name} differ from the serial answer in {int(rows.sum())} of {len(a)} queries (first: {int(rows.argmax())})")


def _assert_oracle(got, ref, what):
    """keys, distance bits, counts and the first three stats columns (evaluations, base hops, upper hops) against the oracle's walk"""
    ok, od, oc, ost = ref
    assert (got[2] == oc).all(), what
    assert (got[0] == ok).all(), f"{what}: ids differ from the oracle's in {(got[0] != ok).any(axis=1).sum()} queries"
    assert (got[1] == od.view(np.uint32)).all(), what
    if len(got) > 3:
        assert (got[3][:, :3] == ost[:, :3]).all(), what


def _serial(la, nsets, make_out, fire):
    """set j on the null stream, then la.sync(): [answers of set j], seconds"""
    res, t0 = [], time.perf_counter()
    for j in range(nsets):
        o = make_out()
        fire(j, None, o)
        la.sync()
        res.append(o.host())
    return res, time.perf_counter() - t0


def _overlapped(la, streams, nsets, rounds, make_out, fire):
    """round r: stream i gets set (i + r) % nsets; nothing waits until the one la.sync() at the end.  [(set of the last round, stream
    i's buffers)], seconds per round"""
    outs = [make_out() for _ in streams]
    la.sync()  # the prefill of the buffers (null stream) is not what is under test
    t0 = time.perf_counter()
    for r in range(rounds):
        for i, st in enumerate(streams):
            fire((i + r) % nsets, st, outs[i])
    la.sync()
    dt = (time.perf_counter() - t0) / rounds
    return [((i + rounds - 1) % nsets, o.host()) for i, o in enumerate(outs)], dt


def _leg(la, what, nstreams, nsets, rounds, make_out, fire, oracle=None):
    """serial answers (held to the oracle's, if given), the overlapped rounds, the comparison; returns the serial answers"""
    serial, ts = _serial(la, nsets, make_out, fire)
    if oracle is not None:
        for j in range(nsets):
            _assert_oracle(serial[j], oracle(j), f"{what}, set {j}, null stream")
    with HipStreams(la, nstreams) as st:
        got, tc = _overlapped(la, st, nsets, rounds, make_out, fire)
    print(f"{what}: {nsets} serial calls {ts * 1e3:.2f} ms; one round of {nstreams} calls on {nstreams} streams {tc * 1e3:.2f} ms")
    for i, (j, g) in enumerate(got):
        _assert_same(g, serial[j], f"{what}, stream {i}, set {j}")
    return serial


def _twin(po, s, X):
    g = s.graph_export()
    return po.Graph.from_arrays(X, g["M"], g["M0"], g["max_level"], g["entry"], g["levels"], g["upper_off"], g["adj0"], g["adjU"])


def _knob(la, monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, str(value))
    la.lib().leann_debug_reload_env()


# ---- 1. plain f32 HNSW handle -----------------------------------------------------------------------------------------------------------
class _Plain:
    N, D, M = 20_000, 128, 16

    def __init__(self, la, po):
        self.X = synth(po, self.N, self.D)
        self.dX = la.DeviceArray.from_host(self.X)
        self.s = la.BackendSearcher.build_device(la.BackendType.Hnsw, self.dX.ptr, self.N, self.D, self.D, self.M, 64)
        self.G = _twin(po, self.s, self.X)
        self._ref = {}

    def oracle(self, name, Q, k=K, ef=EF):
        """the oracle's walk of the exported graph: computed once per named query set, left unchanged"""
        if (name, k, ef) not in self._ref:
            r = self.G.search_batch(Q, k, ef, 0, nthreads=8)
            for a in r:
                a.setflags(write=False)
            self._ref[name, k, ef] = r
        return self._ref[name, k, ef]


@pytest.fixture(scope="module")
def plain(la, po, gpu):
    p = _Plain(la, po)
    yield p
    p.s.close()


@pytest.mark.parametrize("nq,nstreams", [(64, 8), (704, 2)])
def test_plain_handle_on_caller_streams(la, po, plain, nq, nstreams):
    """8 sets of 64 queries (16 waves per query, the form that leaves most CUs free) on 8 streams; 2 sets of 704 (4 waves) on 2"""
    Qs = [synth(po, nq, plain.D, stream=1, i0=1000 * t) for t in range(nstreams)]
    dQ = [la.DeviceArray.from_host(Q) for Q in Qs]

    def fire(j, st, o):
        plain.s.search_batch_device(dQ[j].ptr, nq, K, EF, *o.ptrs(), d_stats=o.stats.ptr, stream=st)

    serial = _leg(la, f"plain handle, {nq} queries a call", nstreams, nstreams, 4, lambda: _Out(la, nq, K), fire,
                  oracle=lambda j: plain.oracle(f"{nq}/{j}", Qs[j]))
    assert all((a[2] == K).all() and (a[3][:, 1] > 0).all() for a in serial)  # full answers, every query walked the base layer


def test_queries_produced_on_the_callers_stream(la, po, plain):
    """Each stream's 64 queries are the tail rows of a 200 000-row generation queued on that stream, the search right behind it: any
    part of the library that ran outside the caller's stream would read queries that are not there yet.  Against the oracle's
    answer for the oracle's synth of those rows."""
    nq, rows, S, rounds = 64, 200_000, 8, 3
    tail = (rows - nq) * plain.D * 4
    chk, L = la._native.check, la.lib()
    base = [1_000_000 * (j + 1) for j in range(S)]  # set j: rows [base[j], base[j] + rows) of the query stream
    Qs = [synth(po, nq, plain.D, stream=1, i0=base[j] + rows - nq) for j in range(S)]
    ref = [plain.oracle(f"tail/{j}", Qs[j]) for j in range(S)]
    bufs = [la.DeviceArray((rows, plain.D), np.float32) for _ in range(S)]
    nan = np.full((nq, plain.D), np.nan, np.float32)
    for b in bufs:  # before the first generation lands the tail holds no query at all
        chk(L.leann_device_upload(b.ptr + tail, nan.ctypes.data, nan.nbytes))
    outs = [_Out(la, nq, K) for _ in range(S)]
    la.sync()
    with HipStreams(la, S) as sts:
        t0 = time.perf_counter()
        for r in range(rounds):
            for i, st in enumerate(sts):
                j = (i + r) % S
                chk(L.leann_synth_rows_device(SEED, plain.D, plain.D, 64, 256, 1.0, 1, base[j], rows, bufs[i].ptr, st))
                plain.s.search_batch_device(bufs[i].ptr + tail, nq, K, EF, *outs[i].ptrs(), d_stats=outs[i].stats.ptr, stream=st)
        la.sync()
        print(f"generation + search on {S} streams: {(time.perf_counter() - t0) / rounds * 1e3:.2f} ms a round")
    for i in range(S):
        j = (i + rounds - 1) % S
        Qd = np.empty((nq, plain.D), np.float32)
        chk(L.leann_device_download(Qd.ctypes.data, bufs[i].ptr + tail, Qd.nbytes))
        assert (Qd.view(np.uint32) == Qs[j].view(np.uint32)).all(), (i, j)  # the rows the search was given are the oracle's rows
        _assert_oracle(outs[i].host(), ref[j], f"queries generated on stream {i}, set {j}")


def test_rerank_chained_behind_the_search(la, po, plain):
    """leann_hybrid_rerank_device queued behind the search on the same stream (fetch_k = 50, top_k = 10, up to 64 BM25 positives a
    query, some of them ANN hits): the lists and the reranked answers equal the serial chain's"""
    from test_gpu_hybrid import _sparse_bm25
    nq, S, fetch_k, top_k, stride, alpha = 64, 8, 50, 10, 64, 0.7
    chk, L = la._native.check, la.lib()
    Qs = [synth(po, nq, plain.D, stream=1, i0=1000 * t) for t in range(S)]
    dQ = [la.DeviceArray.from_host(Q) for Q in Qs]

    class Chain:
        def __init__(self):
            self.ann, self.top = _Out(la, nq, fetch_k), _Out(la, nq, top_k, stats=False)

        def host(self):
            return self.ann.host(), self.top.host()

    def search(j, st, o):
        plain.s.search_batch_device(dQ[j].ptr, nq, fetch_k, EF, *o.ann.ptrs(), d_stats=o.ann.stats.ptr, stream=st)

    def rerank(j, st, o):
        chk(L.leann_hybrid_rerank_device(*o.ann.ptrs(), nq, fetch_k, bm[j][0].ptr, bm[j][1].ptr, bm[j][2].ptr, stride, plain.N, alpha, 1, top_k,
                                         *o.top.ptrs(), st))

    rng = np.random.default_rng(64)
    bm, serial = [], []
    for j in range(S):  # the serial chain: search, then the rerank of its lists, both on the null stream
        o = Chain()
        search(j, None, o)
        la.sync()
        ann = o.ann.host()
        _assert_oracle(ann, plain.oracle(f"64/{j}", Qs[j], fetch_k, EF), f"fetch_k = {fetch_k}, set {j}, null stream")
        bm.append([la.DeviceArray.from_host(a) for a in _sparse_bm25(rng, nq, plain.N, stride, ann[0], ann[2], stride)])
        rerank(j, None, o)
        la.sync()
        serial.append(o.host())
        assert (serial[j][1][2] == top_k).all()
    assert any((serial[j][1][0] != serial[j][0][0][:, :top_k]).any() for j in range(S))  # the rerank reorders something

    def fire(j, st, o):
        search(j, st, o)
        rerank(j, st, o)

    with HipStreams(la, S) as sts:
        got, dt = _overlapped(la, sts, S, 3, Chain, fire)
    print(f"search + rerank on {S} streams: {dt * 1e3:.2f} ms a round")
    for i, (j, (ann, top)) in enumerate(got):
        _assert_same(ann, serial[j][0], f"lists, stream {i}, set {j}")
        _assert_same(top, serial[j][1], f"reranked, stream {i}, set {j}")


# ---- 2. visited-set pools under cross-launch contention ---------------------------------------------------------------------------------
def test_visited_set_pools_across_launches(la, po, gpu, monkeypatch):
    """The set-up of test_visited_set_climbs_both_pools_in_both_loop_forms (test_gpu_kernel_matrix.py): a 256-slot LDS table and
    1024-slot pool-1 tables over 5000 i.i.d. rows at ef = 400, so every query moves LDS -> pool 1 -> pool 2.  That test holds 704
    workgroups in contention inside one launch; this one holds 8 x 64 at once across launches of one handle, plain and under a
    shared 10 % bitmap: tables, locks and generations must stay separate between launches."""
    n, d, m, k, ef, nq, S = 5000, 128, 16, 10, 400, 64, 8
    X = synth(po, n, d, r=0)
    Qs = [synth(po, nq, d, stream=1, r=0, i0=1000 * t) for t in range(S)]
    G = po.Graph.build_hnsw(X, M=m, efc=64)
    bm = np.packbits(np.random.default_rng(7).random(n) < 0.10, bitorder="little")
    ref = {}
    for name in ("plain", "shared"):  # on the oracle's own numbers, before the GPU is touched: no query can stay below pool 2
        for j in range(S):
            r = ref[name, j] = G.search_batch(Qs[j], k, ef, 0, nthreads=8) if name == "plain" else G.search_filtered_batch(Qs[j], k, ef, bm, 0, nthreads=8)
            assert int(r[3][:, 0].min()) > 1024, (name, j, int(r[3][:, 0].min()))
    _knob(la, monkeypatch, "LEANN_DEBUG_HASH_BITS", 8)    # LDS table: 256 slots
    _knob(la, monkeypatch, "LEANN_DEBUG_GPOOL_BITS", 10)  # pool 1: 1024 slots (the pools are sized at a handle's first use)
    lv, uo, a0, aU = G.export()
    s = la.BackendSearcher.from_arrays(la.BackendType.Hnsw, X, m, 2 * m, G.max_level, G.entry, lv, uo, a0, aU)
    try:
        dQ, dbm = [la.DeviceArray.from_host(Q) for Q in Qs], la.DeviceArray.from_host(bm)
        for name in ("plain", "shared"):
            def fire(j, st, o):
                if name == "plain":
                    s.search_batch_device(dQ[j].ptr, nq, k, ef, *o.ptrs(), d_stats=o.stats.ptr, stream=st)
                else:
                    s.search_filtered_batch_device(dQ[j].ptr, nq, k, ef, dbm.ptr, 0, *o.ptrs(), d_stats=o.stats.ptr, stream=st)

            serial, ts = _serial(la, S, lambda: _Out(la, nq, k), fire)
            for j in range(S):
                _assert_oracle(serial[j], ref[name, j], f"tiny tables, {name}, set {j}, null stream")
            with HipStreams(la, S) as sts:
                got, dt = _overlapped(la, sts, S, 3, lambda: _Out(la, nq, k), fire)
            print(f"tiny tables, {name}: {S} serial calls {ts * 1e3:.2f} ms; {S} x {nq} queries in flight, {dt * 1e3:.2f} ms a round")
            for i, (j, g) in enumerate(got):
                _assert_same(g, serial[j], f"tiny tables, {name}, stream {i}, set {j}")
                assert (g[3][:, 3] == 2).all(), (name, i)  # visited-set level: 0 LDS, 1 pool 1, 2 pool 2
    finally:
        s.close()
        _knob(la, monkeypatch, "LEANN_DEBUG_GPOOL_BITS", None)
        _knob(la, monkeypatch, "LEANN_DEBUG_HASH_BITS", None)


# ---- 3. live mask and caller bitmaps ----------------------------------------------------------------------------------------------------
def test_live_mask_under_different_bitmaps_per_stream(la, po, gpu):
    """300 keys removed and not consolidated: every filtered walk runs under live AND the caller's bitmap, which the library writes
    into a scratch buffer of the stream.  Six streams, each under a different bitmap (about 30 % allowed): a buffer shared between
    streams would AND one stream's bitmap into another's answer.  Then one bitmap per query, 16 queries a call."""
    n, d, m, S = 4000, 128, 16, 6
    X = synth(po, n, d)
    dX = la.DeviceArray.from_host(X)
    s = la.BackendSearcher.build_device(la.BackendType.Hnsw, dX.ptr, n, d, d, m, 64)
    gone = np.random.default_rng(300).choice(n, size=300, replace=False).astype(np.uint64)
    assert s.remove(gone) == 300
    live = np.ones(n, bool)
    live[gone.astype(np.int64)] = False
    stride = (n + 7) // 8
    for form, nq in (("shared", 64), ("per query", 16)):
        Qs = [synth(po, nq, d, stream=1, i0=1000 * t) for t in range(S)]
        bits = [np.random.default_rng(1000 + t).random((nq, n) if form == "per query" else n) < 0.30 for t in range(S)]
        dQ = [la.DeviceArray.from_host(Q) for Q in Qs]
        dA = [la.DeviceArray.from_host(np.packbits(b, axis=-1, bitorder="little")) for b in bits]
        assert dA[0].shape[-1] == stride

        def fire(j, st, o):
            s.search_filtered_batch_device(dQ[j].ptr, nq, K, EF, dA[j].ptr, stride if form == "per query" else 0, *o.ptrs(),
                                           d_stats=o.stats.ptr, stream=st)

        serial = _leg(la, f"removals + {form} bitmaps", S, S, 4, lambda: _Out(la, nq, K), fire)
        for j, (keys, _, counts, stats) in enumerate(serial):
            assert (counts == K).all() and (stats[:, 1] > 0).all(), (form, j)
            pos = keys.astype(np.int64)
            assert live[pos].all(), (form, j)  # no returned key is a removed one
            allowed = bits[j][np.arange(nq)[:, None], pos] if form == "per query" else bits[j][pos]
            assert allowed.all(), (form, j)
        assert len({a[0].tobytes() for a in serial}) == S  # the sets' answers differ: a mixed-up buffer cannot pass
    s.close()


# ---- 4. recompute-on graph handles ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [256, 100])
def test_recompute_on_graph_projects_into_the_streams_own_scratch(la, po, gpu, h):
    """The walk of a recompute-on handle runs on g = W q, projected into a scratch buffer of the stream (h = 256: the
    four-rows-per-instruction reader; h = 100: the general one).  6 streams x 64 different queries, uploaded and then generated on
    the stream; then 64, 704 and 64 queries queued on one fresh stream, whose scratch has to grow between two queued calls."""
    n, d, deg, S, nq = 4000, 128, 16, 6, 64
    Lc, chk = la.lib(), la._native.check
    F = po.synth_features(SEED, h, 64, 1.0, 0, 0, n)
    W = po.synth_weights(SEED, h, d)
    Q = po.recompute_encode(po.synth_features(SEED, h, 64, 1.0, 1, 0, 704), W)
    dF, dW = la.DeviceArray.from_host(F), la.DeviceArray.from_host(W)
    r, hb = C.c_void_p(), C.c_void_p()
    chk(Lc.leann_recompute_create(dF.ptr, n, h, dW.ptr, d, 0, 0, C.byref(r)))
    chk(Lc.leann_recompute_build_index(r, 0, deg, 64, C.byref(hb)))
    s = la.BackendSearcher(hb, la.BackendType.Hnsw)
    dQ = [la.DeviceArray.from_host(Q[nq * t: nq * (t + 1)]) for t in range(S)]

    def fire(j, st, o):
        s.search_batch_device(dQ[j].ptr, nq, K, EF, *o.ptrs(), d_stats=o.stats.ptr, stream=st)

    serial = _leg(la, f"recompute-on graph, h = {h}", S, S, 4, lambda: _Out(la, nq, K), fire)
    assert all((a[2] == K).all() for a in serial) and len({a[0].tobytes() for a in serial}) == S
    # the same with each stream's 64 queries generated on that stream first (the tail rows of 200 000, as in
    # test_queries_produced_on_the_callers_stream): while the generations run the host queues every stream's projection and walk, so
    # these then run side by side on the device, not one after the other at the pace the host issues them
    rows = 200_000
    tail = (rows - nq) * d * 4
    pool = itertools.cycle([la.DeviceArray((rows, d), np.float32) for _ in range(S)])

    def gen_out():
        o = _Out(la, nq, K)
        o.buf = next(pool)
        return o

    def fire_gen(j, st, o):
        chk(Lc.leann_synth_rows_device(SEED, d, d, 64, 256, 1.0, 1, 1_000_000 * (j + 1), rows, o.buf.ptr, st))
        s.search_batch_device(o.buf.ptr + tail, nq, K, EF, *o.ptrs(), d_stats=o.stats.ptr, stream=st)

    gen = _leg(la, f"recompute-on graph, h = {h}, queries generated on the stream", S, S, 3, gen_out, fire_gen)
    assert all((a[2] == K).all() for a in gen) and len({a[0].tobytes() for a in gen}) == S
    # one stream, three queued calls of 64, 704 and 64 queries
    dAll = la.DeviceArray.from_host(Q)
    calls = [(dQ[1], 64), (dAll, 704), (dQ[2], 64)]
    want = []
    for q, m in calls:
        o = _Out(la, m, K)
        s.search_batch_device(q.ptr, m, K, EF, *o.ptrs(), d_stats=o.stats.ptr)
        la.sync()
        want.append(o.host())
    outs = [_Out(la, m, K) for _, m in calls]
    la.sync()
    with HipStreams(la, 1) as sts:
        for (q, m), o in zip(calls, outs):
            s.search_batch_device(q.ptr, m, K, EF, *o.ptrs(), d_stats=o.stats.ptr, stream=sts[0])
        la.sync()
    for (q, m), o, w in zip(calls, outs, want):
        _assert_same(o.host(), w, f"h = {h}: {m} queries, one stream")
    _assert_same(want[0], serial[1], "the same set twice on the null stream")
    s.close()
    Lc.leann_recompute_close(r)


# ---- 5. row screen ----------------------------------------------------------------------------------------------------------------------
def test_row_screen_counters_add_up_across_streams(la, po, gpu):
    """4000 x 768, two clusters (the smallest screening shape of test_gpu_row_screen.py), screen on, 3 streams x 704 queries at
    ef = 56.  The ruled-out / read-in-full counters are device atomics shared by all launches of the handle: their increment over
    the overlapped rounds is the sum of the serial increments of the calls those rounds made."""
    n, d, m, nq, S, ef, rounds = 4000, 768, 16, 704, 3, 56, 2
    X = synth(po, n, d, n_clusters=2)
    dX = la.DeviceArray.from_host(X)
    s = la.BackendSearcher.build_device(la.BackendType.Hnsw, dX.ptr, n, d, d, m, 64)
    s.set_row_screen(True)
    Qs = [synth(po, nq, d, stream=1, n_clusters=2, i0=1000 * t) for t in range(S)]
    dQ = [la.DeviceArray.from_host(Q) for Q in Qs]
    G = _twin(po, s, X)

    def fire(j, st, o):
        s.search_batch_device(dQ[j].ptr, nq, K, ef, *o.ptrs(), d_stats=o.stats.ptr, stream=st)

    serial, inc = [], []
    for j in range(S):
        c0 = s.row_screen_stats()
        o = _Out(la, nq, K)
        fire(j, None, o)
        la.sync()
        c1 = s.row_screen_stats()
        serial.append(o.host())
        inc.append({f: c1[f] - c0[f] for f in c0})
        _assert_oracle(serial[j], G.search_batch(Qs[j], K, ef, 0, nthreads=8), f"row screen, set {j}, null stream")
        assert inc[j]["ruled_out"] > 0  # the screening kernel ran
        assert inc[j]["ruled_out"] + inc[j]["read_in_full"] == int(serial[j][3][:, 0].sum()) - nq  # every evaluation but the entry points
    c0 = s.row_screen_stats()
    with HipStreams(la, S) as sts:
        got, dt = _overlapped(la, sts, S, rounds, lambda: _Out(la, nq, K), fire)
    c1 = s.row_screen_stats()
    print(f"row screen: {S} x {nq} queries in flight, {dt * 1e3:.2f} ms a round; serial increments {inc}")
    for i, (j, g) in enumerate(got):
        _assert_same(g, serial[j], f"row screen, stream {i}, set {j}")
    for f in ("ruled_out", "read_in_full"):  # every round runs every set once
        assert c1[f] - c0[f] == rounds * sum(x[f] for x in inc), f
    s.close()


# ---- 6. bf16 rows -----------------------------------------------------------------------------------------------------------------------
def test_bf16_row_handle_on_caller_streams(la, po, gpu):
    import bf16_ref
    n, d, m, S, nq = 4000, 128, 16, 4, 64
    X = synth(po, n, d)
    dX = la.DeviceArray.from_host(X)
    s = la.BackendSearcher.build_device(la.BackendType.Hnsw, dX.ptr, n, d, d, m, 64, row_type=la.RowType.BF16)
    assert s.row_type() == la.RowType.BF16
    G = _twin(po, s, bf16_ref.rounded(X))  # the index is the f32 index over the rounded rows
    Qs = [synth(po, nq, d, stream=1, i0=1000 * t) for t in range(S)]
    dQ = [la.DeviceArray.from_host(Q) for Q in Qs]

    def fire(j, st, o):
        s.search_batch_device(dQ[j].ptr, nq, K, EF, *o.ptrs(), d_stats=o.stats.ptr, stream=st)

    _leg(la, "bf16 rows", S, S, 4, lambda: _Out(la, nq, K), fire, oracle=lambda j: G.search_batch(Qs[j], K, EF, 0, nthreads=8))
    s.close()


# ---- 7. synchronous scan-type calls from threads with their own streams -----------------------------------------------------------------
def _threads(la, T, rounds, work):
    """T host threads, each with a non-blocking stream of its own: work(t, r, stream) for r in range(rounds); the first error is raised"""
    errors = []

    def run(t, st):
        try:
            for r in range(rounds):
                work(t, r, st)
        except BaseException as e:  # noqa: BLE001
            errors.append((t, e))

    with HipStreams(la, T) as sts:
        th = [threading.Thread(target=run, args=(t, sts[t])) for t in range(T)]
        t0 = time.perf_counter()
        [x.start() for x in th]
        [x.join() for x in th]
        la.sync()
        dt = time.perf_counter() - t0
    if errors:
        raise errors[0][1]
    return dt


def test_exact_scan_from_threads_shares_the_scratch_pool(la, po, gpu):
    """leann_scan_topk_device, the shapes of test_recycled_scratch_is_never_read_before_it_is_written (test_gpu_robust.py), from 4
    threads x 3 rounds.  Each thread walks the shape list from another offset, so blocks of the process-wide scratch pool change
    hands between threads while other scans are in flight."""
    d, T, rounds = 96, 4, 3
    chk, L = la._native.check, la.lib()
    X = synth(po, 70_000, d)
    dX = la.DeviceArray.from_host(X)
    shapes = [(70_000, 64, 10), (3_000, 3, 2), (66_000, 17, 64), (2_049, 1, 1), (70_000, 5, 100), (4_100, 64, 10), (70_000, 64, 10)]
    Qs = [synth(po, nq, d, stream=1, i0=n + 7 * i) for i, (n, nq, k) in enumerate(shapes)]
    dQ = [la.DeviceArray.from_host(Q) for Q in Qs]

    def scan(i, st, o):
        n, nq, k = shapes[i]
        chk(L.leann_scan_topk_device(dX.ptr, n, d, d, dQ[i].ptr, nq, k, None, 0, *o.ptrs(), st))

    hip = HipStreams(la, 0)  # the runtime only: each thread synchronises the stream _threads gives it
    serial, t0 = [], time.perf_counter()
    for i, (n, nq, k) in enumerate(shapes):
        o = _Out(la, nq, k, stats=False)
        scan(i, None, o)
        la.sync()
        serial.append(o.host())
        for q in range(0, nq, max(1, nq // 4)):  # ... and the serial answer against the oracle's scan, on sampled queries
            k0, s0 = po.scan_topk(X[:n], Qs[i][q], k, mode=1)
            assert (serial[i][0][q] == k0).all() and (serial[i][1][q] == np.asarray(s0, np.float32).view(np.uint32)).all(), (n, nq, k, q)
    ts = time.perf_counter() - t0
    outs = [[_Out(la, nq, k, stats=False) for n, nq, k in shapes] for _ in range(T)]
    got = [[[None] * len(shapes) for _ in range(rounds)] for _ in range(T)]
    la.sync()

    def work(t, r, st):
        for step in range(len(shapes)):
            i = (2 * t + r + step) % len(shapes)
            outs[t][i].poison()
            scan(i, st, outs[t][i])
            hip.synchronize(st)  # the call is synchronous; this only orders the download below behind it by the book
            got[t][r][i] = outs[t][i].host()

    dt = _threads(la, T, rounds, work)
    print(f"exact scan: {len(shapes)} serial calls (+ oracle) {ts * 1e3:.1f} ms; {T} threads x {rounds} rounds x {len(shapes)} calls {dt * 1e3:.1f} ms")
    for t in range(T):
        for r in range(rounds):
            for i in range(len(shapes)):
                _assert_same(got[t][r][i], serial[i], f"scan {shapes[i]}, thread {t}, round {r}")


def test_exact_filtered_search_from_threads(la, po, gpu):
    """search_filtered_exact_batch_device on a 20 000 x 96 handle under 2 % bitmaps, one shared and one per query, from 4 threads x 3
    rounds; the sets rotate over the threads"""
    n, d, T, rounds, nq, k = 20_000, 96, 4, 3, 24, 10
    X = synth(po, n, d)
    dX = la.DeviceArray.from_host(X)
    s = la.BackendSearcher.build_device(la.BackendType.Hnsw, dX.ptr, n, d, d, 16, 64)
    stride = (n + 7) // 8
    Qs = [synth(po, nq, d, stream=1, i0=1000 * t) for t in range(T)]
    dQ = [la.DeviceArray.from_host(Q) for Q in Qs]
    bits = {("shared", j): np.random.default_rng(50 + j).random(n) < 0.02 for j in range(T)}
    bits.update({("per query", j): np.random.default_rng(60 + j).random((nq, n)) < 0.02 for j in range(T)})
    dA = {key: la.DeviceArray.from_host(np.packbits(b, axis=-1, bitorder="little")) for key, b in bits.items()}
    forms = ("shared", "per query")

    def call(form, j, st, o):
        s.search_filtered_exact_batch_device(dQ[j].ptr, nq, k, dA[form, j].ptr, stride if form == "per query" else 0, *o.ptrs(), stream=st)

    serial = {}
    for form in forms:
        for j in range(T):
            o = _Out(la, nq, k, stats=False)
            call(form, j, None, o)
            la.sync()
            keys, dist_bits, counts = serial[form, j] = o.host()
            assert (counts == k).all()
            pos = keys.astype(np.int64)
            assert (bits[form, j][np.arange(nq)[:, None], pos] if form == "per query" else bits[form, j][pos]).all(), (form, j)
    assert len({serial[form, j][0].tobytes() for form in forms for j in range(T)}) == 2 * T  # eight different answers
    hip = HipStreams(la, 0)
    outs = [{form: _Out(la, nq, k, stats=False) for form in forms} for _ in range(T)]
    got = [[{} for _ in range(rounds)] for _ in range(T)]
    la.sync()

    def work(t, r, st):
        j = (t + r) % T
        for form in forms:
            outs[t][form].poison()
            call(form, j, st, outs[t][form])
            hip.synchronize(st)
            got[t][r][form] = (j, outs[t][form].host())

    dt = _threads(la, T, rounds, work)
    print(f"exact filtered search: {T} threads x {rounds} rounds x 2 calls {dt * 1e3:.1f} ms")
    for t in range(T):
        for r in range(rounds):
            for form in forms:
                j, g = got[t][r][form]
                _assert_same(g, serial[form, j], f"exact filtered, {form}, thread {t}, round {r}, set {j}")
    s.close()


def test_recompute_search_from_threads(la, po, gpu):
    """leann_recompute_search_batch_device (encode + score + top-k, no stored vectors) on 3000 passages, h = 64, d = 128, from 4
    threads x 3 rounds; the sets rotate over the threads"""
    n, h, d, T, rounds, nq, k = 3000, 64, 128, 4, 3, 33, 10
    Lc, chk = la.lib(), la._native.check
    F = po.synth_features(SEED, h, 64, 1.0, 0, 0, n)
    W = po.synth_weights(SEED, h, d)
    Q = po.recompute_encode(po.synth_features(SEED, h, 64, 1.0, 1, 0, T * nq), W)
    dF, dW = la.DeviceArray.from_host(F), la.DeviceArray.from_host(W)
    dQ = [la.DeviceArray.from_host(Q[nq * t: nq * (t + 1)]) for t in range(T)]
    rc = C.c_void_p()
    chk(Lc.leann_recompute_create(dF.ptr, n, h, dW.ptr, d, 0, 0, C.byref(rc)))

    def call(j, st, o):
        chk(Lc.leann_recompute_search_batch_device(rc, dQ[j].ptr, nq, k, None, *o.ptrs(), st))

    serial = _serial(la, T, lambda: _Out(la, nq, k, stats=False), call)[0]
    assert all((a[2] == k).all() for a in serial) and len({a[0].tobytes() for a in serial}) == T
    hip = HipStreams(la, 0)
    outs = [_Out(la, nq, k, stats=False) for _ in range(T)]
    got = [[None] * rounds for _ in range(T)]
    la.sync()

    def work(t, r, st):
        j = (t + r) % T
        outs[t].poison()
        call(j, st, outs[t])
        hip.synchronize(st)
        got[t][r] = (j, outs[t].host())

    dt = _threads(la, T, rounds, work)
    print(f"recompute search: {T} threads x {rounds} rounds {dt * 1e3:.1f} ms")
    for t in range(T):
        for r in range(rounds):
            j, g = got[t][r]
            _assert_same(g, serial[j], f"recompute search, thread {t}, round {r}, set {j}")
    Lc.leann_recompute_close(rc)


# ---- 8. composite handle ----------------------------------------------------------------------------------------------------------------
class _Composite:
    N, D, M = 6016, 64, 16

    def __init__(self, la, po):
        X = synth(po, self.N, self.D)
        lows = [0, 3008, self.N]  # two shards on one device, the boundary a multiple of 64 (test_gpu_bm25.py)
        self.parts = [la.DeviceArray.from_host(X[lows[g]:lows[g + 1]]) for g in range(2)]
        self.sh = la.ShardedIndex.build_device(la.BackendType.Hnsw, [p.ptr for p in self.parts], [lows[g + 1] - lows[g] for g in range(2)],
                                               self.D, self.D, self.M, 48, [0, 0], keep=self.parts)
        self.Qs = [synth(po, 200, self.D, stream=1, i0=1000 * t) for t in range(3)]
        self.dQ = [la.DeviceArray.from_host(Q) for Q in self.Qs]
        self._serial, self.seconds = {}, {}

    def serial(self, la, j, nq, stats):
        """the first nq queries of set j through the synchronous entry point on the null stream, local branch: computed once"""
        if (j, nq, stats) not in self._serial:
            o = _Out(la, nq, K, stats=stats)
            la.sync()
            t0 = time.perf_counter()
            self.sh.search_batch_device(self.dQ[j].ptr, nq, K, 48, *o.ptrs(), d_stats=o.stats.ptr if stats else None)
            la.sync()
            self.seconds[j, nq, stats] = time.perf_counter() - t0
            self._serial[j, nq, stats] = o.host()
            assert (self._serial[j, nq, stats][0] >= 3008).any() and (self._serial[j, nq, stats][0] < 3008).any()  # both shards answer
        return self._serial[j, nq, stats]


@pytest.fixture(scope="module")
def composite(la, po, gpu):
    c = _Composite(la, po)
    yield c
    c.sh.close()


@pytest.mark.parametrize("remote", [False, True], ids=["local", "forced-remote"])
@pytest.mark.parametrize("stats", [False, True], ids=["no-stats", "stats"])
def test_composite_handle_more_calls_than_slots(la, composite, monkeypatch, stats, remote):
    """search_batch_device of a two-shard handle from 3 caller streams x 3 rounds with no host synchronisation: nine calls behind the two
    rotating result slots.  The streams ask for 20, 64 and 200 queries, so the slot buffers grow while earlier calls are queued.
    forced-remote (LEANN_DEBUG_FORCE_REMOTE=1, as test_remote_shard_branch_on_one_device) routes through the per-shard staging
    buffers; its answers are held to the local branch's serial ones."""
    c, nqs, rounds = composite, (20, 64, 200), 3
    want = {(i, (i + rounds - 1) % 3): c.serial(la, (i + rounds - 1) % 3, nqs[i], stats) for i in range(3)}  # the last round's calls
    outs = [_Out(la, nq, K, stats=stats) for nq in nqs]
    la.sync()
    if remote:
        _knob(la, monkeypatch, "LEANN_DEBUG_FORCE_REMOTE", 1)
    with HipStreams(la, 3) as sts:
        t0 = time.perf_counter()
        for r in range(rounds):
            for i, st in enumerate(sts):
                c.sh.search_batch_device(c.dQ[(i + r) % 3].ptr, nqs[i], K, 48, *outs[i].ptrs(), d_stats=outs[i].stats.ptr if stats else None, stream=st)
        la.sync()
        tc, ts = time.perf_counter() - t0, sum(c.seconds[j, nqs[i], stats] for i, j in want)
        print(f"composite handle: 3 serial calls {ts * 1e3:.2f} ms; {3 * rounds} calls on 3 streams {tc * 1e3:.2f} ms")
    for i in range(3):
        j = (i + rounds - 1) % 3
        _assert_same(outs[i].host(), want[i, j], f"composite handle, stream {i} ({nqs[i]} queries), set {j}")


@pytest.mark.parametrize("remote", [False, True], ids=["local", "forced-remote"])
def test_composite_tickets_behind_different_streams(la, composite, monkeypatch, remote):
    """Ticket form: the queries of tickets t and t + 1 arrive on two different streams (a device-to-device copy queued right before
    the call), wait() puts both behind a third stream, and the download is queued behind that third stream only."""
    c, nq = composite, 64
    want = [c.serial(la, j, nq, True) for j in (0, 1)]
    qbytes = nq * c.D * 4
    dq = [la.DeviceArray.from_host(np.full((nq, c.D), np.nan, np.float32)) for _ in range(2)]  # no query yet
    outs = [_Out(la, nq, K) for _ in range(2)]
    host = [(np.zeros((nq, K), np.uint64), np.zeros((nq, K), np.uint32), np.zeros(nq, np.uint32), np.zeros((nq, 4), np.uint32)) for _ in range(2)]
    la.sync()
    if remote:
        _knob(la, monkeypatch, "LEANN_DEBUG_FORCE_REMOTE", 1)
    with HipStreams(la, 3) as sts:
        tickets = []
        for i in range(2):
            sts.copy_async(dq[i].ptr, c.dQ[i].ptr, qbytes, sts.D2D, sts[i])
            tickets.append(c.sh.search_batch_device_async(dq[i].ptr, nq, K, 48, *outs[i].ptrs(), d_stats=outs[i].stats.ptr, stream=sts[i]))
        assert tickets[1] == tickets[0] + 1
        for t in tickets:
            c.sh.wait(t, stream=sts[2])
        for i in range(2):
            for a, dev in zip(host[i], (outs[i].keys, outs[i].dists, outs[i].counts, outs[i].stats)):
                sts.copy_async(a.ctypes.data, dev.ptr, a.nbytes, sts.D2H, sts[2])
        sts.synchronize(sts[2])
        for i in range(2):
            _assert_same(host[i], want[i], f"ticket {tickets[i]}, downloaded behind the waiting stream")
        la.sync()


# ---- 9. graph replay, in a child process ------------------------------------------------------------------------------------------------
def test_hip_graph_replay_of_eight_forked_calls(po, gpu, tmp_path):
    """tests/stream_graph_child.py captures fork -> 8 calls of 64 queries on 8 streams -> join into a HIP graph and replays it three
    times over changing query contents; the same 24 (set, buffer) calls run uncaptured on the null stream.  INTEGRATION.md promises
    capturability, so a capture or replay error is a failure, with its text."""
    here = os.path.dirname(os.path.abspath(__file__))
    out = tmp_path / "graph.npz"
    r = subprocess.run([sys.executable, os.path.join(here, "stream_graph_child.py"), str(out)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, f"child exited {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    z = np.load(out)
    for name in ("keys", "dist_bits", "counts", "stats"):  # [replay, buffer, 64, ..] each
        a, b = z["graph_" + name], z["plain_" + name]
        assert a.shape == b.shape and a.shape[:3] == (3, 8, 64), name
        assert a.tobytes() == b.tobytes(), f"{name}: replayed != uncaptured in (replay, buffer) {sorted(set(zip(*np.nonzero(a != b)[:2])))}"
    assert len({z["plain_keys"][r_, b].tobytes() for r_ in range(3) for b in range(8)}) == 24  # 24 different answers
    X, Q = synth(po, 20_000, 128), z["queries"]  # [sets, 64, 128]: the child's query sets; (replay r, buffer b) ran set z["sets"][r, b]
    assert (Q[0].view(np.uint32) == synth(po, 64, 128, stream=1).view(np.uint32)).all()
    G = po.Graph.from_arrays(X, int(z["M"]), int(z["M0"]), int(z["max_level"]), int(z["entry"]), z["levels"], z["upper_off"], z["adj0"], z["adjU"])
    r_, b = 2, 5
    j = int(z["sets"][r_, b])
    got = tuple(z["graph_" + name][r_, b] for name in ("keys", "dist_bits", "counts", "stats"))
    _assert_oracle(got, G.search_batch(Q[j], K, EF, 0, nthreads=8), f"replay {r_}, buffer {b}, set {j}")
