"""-m gpu: recompute search and recompute-on graphs for dims above 768 (up to 4 096, the stored-vector path's limit).
The general encode kernel walks the columns in blocks (recompute_blocked.cuh: feature tile resident in LDS, blocks of 1/2/3/4/6 x 128
columns, sums of squares accumulated block after block); the feature-stationary kernel takes more than six weight sub-slices.
Against the oracle restatement of src/index/recompute.rs:86-109 with the provider tail of src/embedding/candle.rs:165,218-225, with
the tolerances of tests/test_gpu_recompute.py: embeddings 1e-6 (2e-6 pooled), row norms 1e-5, scores 1e-5, ids equal except across
oracle near-ties (<= 2e-5) — and the oracle's own lists may hold such a near-tie in at most 2 % of their (query, rank) pairs, checked
before the GPU's answer is looked at, so that the exception cannot hide a wrong kernel."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = 0x5EED0001
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "leann-rs_amd", "host", "leann")

_REF = {}  # (n, h, d) -> (F, W, E): one oracle pass per shape, shared by the tests and never written to


def _ref(po, n, h, d):
    key = (n, h, d)
    if key not in _REF:
        F = po.synth_features(SEED, h, 64, 1.0, 0, 0, n)
        W = po.synth_weights(SEED, h, d)
        E = po.recompute_encode(F, W)
        for a in (F, W, E):
            a.setflags(write=False)
        _REF[key] = (F, W, E)
    return _REF[key]


def _queries(po, W, h, nq):
    return po.recompute_encode(po.synth_features(SEED, h, 64, 1.0, 1, 0, nq), W)  # embeddings of query-side features


def _create(la, dF, n, h, dW, d, key_offset=0):
    r = C.c_void_p()
    la._native.check(la.lib().leann_recompute_create(dF.ptr, n, h, dW.ptr, d, 0, key_offset, C.byref(r)))
    return r


def _search(la, r, dQ, nq, k, dM=None):
    L, chk = la.lib(), la._native.check
    dk, ds, dc = la.DeviceArray((nq, k), np.uint64), la.DeviceArray((nq, k), np.float32), la.DeviceArray(nq, np.uint32)
    chk(L.leann_recompute_search_batch_device(r, dQ.ptr, nq, k, dM.ptr if dM is not None else None, dk.ptr, ds.ptr, dc.ptr, None))
    la.sync()
    return dk.to_host(), ds.to_host(), dc.to_host()


def _encode(la, r, n, d):
    ld = (d + 3) // 4 * 4
    dE = la.DeviceArray((n, ld), np.float32)
    la._native.check(la.lib().leann_recompute_encode_device(r, 0, n, dE.ptr, None))
    la.sync()
    return dE.to_host()


ENCODE_SHAPES = [(300, 256, 769),     # first width past the old limit, ld = 772: blocks 6 + 1, the last one almost all padding
                 (1300, 256, 896),    # seven column tiles
                 (1500, 256, 1024), (1500, 256, 1536),
                 (900, 100, 1000),    # h not a multiple of 16, d not a multiple of 128
                 (700, 64, 3072), (600, 128, 4096)]  # no n is a multiple of 128: the tail tile runs


@pytest.mark.parametrize("n,h,d", ENCODE_SHAPES)
def test_wide_encode_matches_oracle(la, po, gpu, n, h, d):
    F, W, ref = _ref(po, n, h, d)
    dF, dW = la.DeviceArray.from_host(F), la.DeviceArray.from_host(W)
    r = _create(la, dF, n, h, dW, d)
    full = _encode(la, r, n, d)
    E = full[:, :d]
    print(f"encode {n}x{h}x{d}: max |E - oracle| = {np.abs(E - ref).max():.3e}, max | |E| - 1 | = {np.abs(np.linalg.norm(E, axis=1) - 1).max():.3e}")
    assert np.abs(E - ref).max() <= 1e-6
    assert np.abs(np.linalg.norm(E, axis=1) - 1).max() <= 1e-5
    assert (full[:, d:] == 0).all()  # the padding columns of a row (ld = 772 at d = 769)
    if d == 1536:  # the same input gives the same bits on every run (no atomics in the block-wise sums)
        again = _encode(la, r, n, d)
        assert (again.view(np.uint32) == full.view(np.uint32)).all()
    la.lib().leann_recompute_close(r)


def _near_tie_share(lists, k):
    """share of (query, rank) pairs of the oracle's own lists whose gap to the next rank is <= 2e-5"""
    near = sum(int((s0[:k] - s0[1:k + 1] <= 2e-5).sum()) for _, s0 in lists)
    return near / (len(lists) * k)


def _check_against_lists(gk, gs, lists, k):
    for i, (k0, s0) in enumerate(lists):
        assert np.abs(gs[i] - s0[:k]).max() <= 1e-5
        assert (np.diff(gs[i]) <= 0).all()
        for j in range(k):
            if gk[i, j] != k0[j]:  # only allowed across a near-tie of the oracle's
                assert gk[i, j] in k0 and abs(s0[j] - s0[list(k0).index(gk[i, j])]) <= 2e-5


@pytest.mark.parametrize("n,h,d,nq,k", [(1300, 256, 896, 33, 10), (1500, 256, 1024, 40, 10), (1500, 256, 1536, 70, 10),  # feature-stationary
                                        (900, 100, 1000, 5, 10), (700, 64, 3072, 9, 10), (600, 128, 4096, 3, 5)])       # blocked, fused
def test_wide_search_matches_restatement(la, po, gpu, n, h, d, nq, k):
    F, W, E = _ref(po, n, h, d)
    Q = _queries(po, W, h, nq)
    lists = [po.scan_topk(E, Q[i], k + 5, mode=0) for i in range(nq)]  # dot_product + stable sort desc + take (recompute.rs:96-109)
    assert _near_tie_share(lists, k) <= 0.02  # on the oracle's scores alone
    dF, dW, dQ = la.DeviceArray.from_host(F), la.DeviceArray.from_host(W), la.DeviceArray.from_host(Q)
    r = _create(la, dF, n, h, dW, d)
    gk, gs, gc = _search(la, r, dQ, nq, k)
    assert (gc == k).all()
    _check_against_lists(gk, gs, lists, k)
    la.lib().leann_recompute_close(r)


def test_wide_general_kernel_agrees_with_feature_stationary(la, po, gpu, monkeypatch):
    n, h, d, nq, k = 1500, 256, 1536, 70, 10
    F, W, E = _ref(po, n, h, d)
    Q = _queries(po, W, h, nq)
    dF, dW, dQ = la.DeviceArray.from_host(F), la.DeviceArray.from_host(W), la.DeviceArray.from_host(Q)
    r = _create(la, dF, n, h, dW, d)
    fk, fs, fc = _search(la, r, dQ, nq, k)
    monkeypatch.setenv("LEANN_DEBUG_FUSED_V1", "1")  # the general kernel: two blocks of six column tiles, scores in the second
    la.lib().leann_debug_reload_env()
    vk, vs, vc = _search(la, r, dQ, nq, k)
    monkeypatch.delenv("LEANN_DEBUG_FUSED_V1")
    la.lib().leann_debug_reload_env()
    print(f"general vs feature-stationary at d = {d}: max |score diff| = {np.abs(vs - fs).max():.3e}, equal keys {(vk == fk).mean():.4f}")
    assert (vc == k).all() and (fc == k).all()
    assert np.abs(vs - fs).max() <= 1e-5
    lists = [po.scan_topk(E, Q[i], k + 5, mode=0) for i in range(nq)]
    assert _near_tie_share(lists, k) <= 0.02
    _check_against_lists(vk, vs, lists, k)
    la.lib().leann_recompute_close(r)


@pytest.mark.parametrize("n,h,d", [(1500, 256, 1536),   # a third allowed -> the compacted row-list kernel
                                   (900, 100, 1000)])   # the masked pass of the general kernel
def test_wide_allow_mask_and_offset(la, po, gpu, n, h, d):
    nq, k = 6, 8
    F, W, E = _ref(po, n, h, d)
    Q = _queries(po, W, h, nq)
    dF, dW, dQ = la.DeviceArray.from_host(F), la.DeviceArray.from_host(W), la.DeviceArray.from_host(Q)
    r = _create(la, dF, n, h, dW, d, key_offset=1000000)
    mask = np.zeros((n + 7) // 8, np.uint8)
    for i in range(0, n, 3):
        mask[i >> 3] |= 1 << (i & 7)
    dM = la.DeviceArray.from_host(mask)
    gk, gs, gc = _search(la, r, dQ, nq, k, dM)
    assert (gc == k).all()
    assert (gk >= 1000000).all() and (gk < 1000000 + n).all() and ((gk - 1000000) % 3 == 0).all()
    for i in range(nq):
        k0, s0 = po.scan_topk(E, Q[i], k, mode=0, allow_mask=mask)
        assert np.abs(gs[i] - s0).max() <= 1e-5
    la.lib().leann_recompute_close(r)


def test_wide_masked_mean_pooling_provider(la, po, gpu):
    """token-level provider at d = 1024: dense per token -> masked mean over L = 4 tokens (pooled per column block, before squaring)
    -> l2_normalize; tolerances of test_masked_mean_pooling_provider"""
    n, h, d, nq, k, L = 700, 128, 1024, 20, 10, 4
    Lc, chk = la.lib(), la._native.check
    F = po.synth_features(SEED, h, 64, 1.0, 0, 0, n * L)  # token rows
    W = po.synth_weights(SEED, h, d)
    rng = np.random.default_rng(L)
    mask = (rng.random((n, L)) < 0.7).astype(np.uint8)
    mask[:5] = 0   # fully padded passages: count clamps to 1e-9 -> zero vector
    mask[5:10] = 1
    E = po.recompute_encode_pooled(F, mask, W, L)
    assert np.abs(E[:5]).max() == 0.0
    Q = _queries(po, W, h, nq)
    dF, dW, dM = la.DeviceArray.from_host(F), la.DeviceArray.from_host(W), la.DeviceArray.from_host(mask)
    r = C.c_void_p()
    chk(Lc.leann_recompute_create_pooled(dF.ptr, dM.ptr, n, L, h, dW.ptr, d, 0, 0, C.byref(r)))
    G = _encode(la, r, n, d)
    print(f"pooled encode: max |E - oracle| = {np.abs(G - E).max():.3e}")
    assert np.abs(G - E).max() <= 2e-6
    assert (G[:5] == 0).all()
    gk, gs, gc = _search(la, r, la.DeviceArray.from_host(Q), nq, k)
    for i in range(nq):
        k0, s0 = po.scan_topk(E, Q[i], k, mode=0)
        assert np.abs(gs[i] - s0).max() <= 1e-5
        assert len(set(gk[i].tolist()) & set(k0.tolist())) >= k - 1
    Lc.leann_recompute_close(r)


def test_general_kernel_four_tiles_plain(la, po, gpu):
    """encode_kernel<4, false, false> (encode) and <4, true, false> (search): d = 512 with h = 64, so that the feature-stationary
    kernel (h = 256 only) is not taken; encode_plan(64, 512) is one block of four tiles.  300 token rows: two full tiles and a tail."""
    n, h, d, nq, k = 300, 64, 512, 5, 10
    F, W, ref = _ref(po, n, h, d)
    Q = _queries(po, W, h, nq)
    lists = [po.scan_topk(ref, Q[i], k + 5, mode=0) for i in range(nq)]
    assert _near_tie_share(lists, k) <= 0.02  # on the oracle's scores alone
    dF, dW, dQ = la.DeviceArray.from_host(F), la.DeviceArray.from_host(W), la.DeviceArray.from_host(Q)
    r = _create(la, dF, n, h, dW, d)
    E = _encode(la, r, n, d)
    print(f"encode {n}x{h}x{d}: max |E - oracle| = {np.abs(E - ref).max():.3e}")
    assert np.abs(E - ref).max() <= 1e-6
    assert np.abs(np.linalg.norm(E, axis=1) - 1).max() <= 1e-5
    gk, gs, gc = _search(la, r, dQ, nq, k)
    assert (gc == k).all()
    _check_against_lists(gk, gs, lists, k)
    la.lib().leann_recompute_close(r)


@pytest.mark.parametrize("n,d,L", [(150, 512, 8),   # encode_kernel<4, *, true>: one block of four tiles, lane-partner pooling
                                   (200, 896, 2),   # encode_blocked_kernel<*, true>, blocks 6 + 1: pair pooling
                                   (100, 896, 8)])  # ... and lane-partner pooling (__shfl_xor(.., 32))
def test_general_kernel_pooling_widths(la, po, gpu, n, d, L):
    """masked mean pooling where test_wide_masked_mean_pooling_provider (L = 4, blocked) and test_masked_mean_pooling_provider
    (d = 384) do not reach: h = 64 keeps the feature-stationary kernel out, encode_plan(64, 512) is one block of four tiles and
    encode_plan(64, 896) the blocks 6 + 1; no count of token rows is a multiple of 128.  Tolerances of those two tests."""
    h, nq, k = 64, 20, 10
    Lc, chk = la.lib(), la._native.check
    F = po.synth_features(SEED, h, 64, 1.0, 0, 0, n * L)  # token rows
    W = po.synth_weights(SEED, h, d)
    rng = np.random.default_rng(L)
    mask = (rng.random((n, L)) < 0.7).astype(np.uint8)
    mask[:5] = 0   # fully padded passages: count clamps to 1e-9 -> zero vector
    mask[5:10] = 1
    E = po.recompute_encode_pooled(F, mask, W, L)
    assert np.abs(E[:5]).max() == 0.0
    Q = _queries(po, W, h, nq)
    dF, dW, dM = la.DeviceArray.from_host(F), la.DeviceArray.from_host(W), la.DeviceArray.from_host(mask)
    r = C.c_void_p()
    chk(Lc.leann_recompute_create_pooled(dF.ptr, dM.ptr, n, L, h, dW.ptr, d, 0, 0, C.byref(r)))
    G = _encode(la, r, n, d)
    print(f"pooled encode {n}x{L}x{h}x{d}: max |E - oracle| = {np.abs(G - E).max():.3e}")
    assert np.abs(G - E).max() <= 2e-6
    assert (G[:5] == 0).all()
    gk, gs, gc = _search(la, r, la.DeviceArray.from_host(Q), nq, k)
    lists = [po.scan_topk(E, Q[i], k, mode=0) for i in range(nq)]
    print(f"pooled search: max |score - oracle| = {max(np.abs(gs[i] - s0).max() for i, (_, s0) in enumerate(lists)):.3e}")
    for i, (k0, s0) in enumerate(lists):
        assert np.abs(gs[i] - s0).max() <= 1e-5
        assert len(set(gk[i].tolist()) & set(k0.tolist())) >= k - 1
    Lc.leann_recompute_close(r)


def test_wide_candidate_emission_across_chunks(la, po, gpu, monkeypatch):
    """40 000 passages at d = 1536: one 16k score-slab chunk, then a chunk that emits its survivors straight from the fused kernel
    (twelve weight sub-slices per unit).  Must equal the slab path bit for bit."""
    n, h, d, nq, k = 40000, 256, 1536, 40, 10
    L, chk = la.lib(), la._native.check
    dF, dW = la.DeviceArray((n, h), np.uint16), la.DeviceArray((h, d), np.uint16)
    chk(L.leann_synth_features_device(SEED, h, 64, 4096, 1.0, 0, 0, n, dF.ptr, None))
    chk(L.leann_synth_weights_device(SEED, h, d, dW.ptr, None))
    W = po.synth_weights(SEED, h, d)
    Q = po.recompute_encode(po.synth_features(SEED, h, 4096, 1.0, 1, 0, nq, r_int=64), W)
    dQ = la.DeviceArray.from_host(Q)
    r = _create(la, dF, n, h, dW, d, key_offset=5000)
    gk, gs, gc = _search(la, r, dQ, nq, k)
    assert (gc == k).all() and (np.diff(gs, axis=1) <= 0).all()
    monkeypatch.setenv("LEANN_DEBUG_NO_EMIT", "1")  # same fused kernel, score slab + segment top-k
    L.leann_debug_reload_env()
    sk, ss, sc = _search(la, r, dQ, nq, k)
    monkeypatch.delenv("LEANN_DEBUG_NO_EMIT")
    L.leann_debug_reload_env()
    assert (gk == sk).all() and (gs.view(np.uint32) == ss.view(np.uint32)).all() and (gc == sc).all()
    assert (gk >= 5000 + 16384).any()  # winners from the emitting chunk as well
    L.leann_recompute_close(r)


def test_wide_sharded_equals_one_handle(la, po, gpu):
    n, h, d, nq, k = 1500, 256, 1024, 40, 10
    L, chk = la.lib(), la._native.check
    F, W, _ = _ref(po, n, h, d)
    Q = _queries(po, W, h, nq)
    dF, dW, dQ = la.DeviceArray.from_host(F), la.DeviceArray.from_host(W), la.DeviceArray.from_host(Q)
    one = _create(la, dF, n, h, dW, d)
    lows = [0, 704, n]
    parts = []
    for g in range(2):
        p = C.c_void_p()
        chk(L.leann_recompute_create(dF.ptr + lows[g] * h * 2, lows[g + 1] - lows[g], h, dW.ptr, d, 0, lows[g], C.byref(p)))
        parts.append(p)
    comp = C.c_void_p()
    chk(L.leann_recompute_create_sharded((C.c_void_p * 2)(*parts), 2, C.byref(comp)))
    assert L.leann_recompute_len(comp) == n
    a, b = _search(la, one, dQ, nq, k), _search(la, comp, dQ, nq, k)
    assert (a[2] == b[2]).all() and (a[0] == b[0]).all() and (a[1].view(np.uint32) == b[1].view(np.uint32)).all()
    L.leann_recompute_close(comp)
    for p in parts + [one]:
        L.leann_recompute_close(p)


GRAPH_N, GRAPH_D, GRAPH_NQ, GRAPH_K = 6000, 1536, 200, 10


def _graph_setup(la, po, h):
    F = po.synth_features(SEED, h, 64, 1.0, 0, 0, GRAPH_N)
    W = po.synth_weights(SEED, h, GRAPH_D)
    Q = _queries(po, W, h, GRAPH_NQ)
    dF, dW = la.DeviceArray.from_host(F), la.DeviceArray.from_host(W)
    r = _create(la, dF, GRAPH_N, h, dW, GRAPH_D)
    return F, W, Q, r, (dF, dW)


@pytest.mark.parametrize("backend,deg,h", [(0, 16, 256), (0, 16, 128), (1, 32, 256)])
def test_wide_recompute_on_graph_search(la, po, gpu, backend, deg, h):
    """Graph index with no stored vectors at d = 1536 (516-byte rows instead of 6 144): (a) GPU traversal == oracle traversal over the
    exported graph and feature bytes, bit for bit; (b) the stored-vector twin built from leann_recompute_encode_device's output has
    the same level-0 lists and answers within 1e-5, >= 99 % equal keys."""
    n, d, nq, k = GRAPH_N, GRAPH_D, GRAPH_NQ, GRAPH_K
    Lc, chk = la.lib(), la._native.check
    F, W, Q, r, keep = _graph_setup(la, po, h)
    hb = C.c_void_p()
    chk(Lc.leann_recompute_build_index(r, backend, deg, 64, C.byref(hb)))
    s = la.BackendSearcher(hb, backend)
    fh, rb = C.c_uint32(0), C.c_uint32(0)
    chk(Lc.leann_backend_feature_rows_export(hb, C.byref(fh), C.byref(rb), None))
    assert fh.value == h and rb.value == 2 * h + 8
    rows = np.zeros((n, rb.value), np.uint8)
    chk(Lc.leann_backend_feature_rows_export(hb, None, None, rows.ctypes.data))
    assert (rows[:, : 2 * h].view(np.uint16) == F).all()
    s.stats(reset=True)
    gk, gd, gc = s.search_batch(Q, k, 64)
    st = s.stats()
    assert st["algorithmic_bytes"] < st["n_dist_evals"] * 600  # 2 h + 8 B per evaluated neighbour, not 6 144
    # (a) oracle over the same graph + feature bytes + projected queries
    g = s.graph_export()
    assert g["dims"] == d
    Gr = po.Graph.from_arrays(np.zeros((n, 1), np.float32), g["M"], g["M0"], g["max_level"], g["entry"], g["levels"], g["upper_off"],
                              g["adj0"], g["adjU"])
    Gr.set_features(rows, fh.value, rb.value)
    ok, od, oc, ost = Gr.search_batch(po.project_queries(W, Q, fh.value), k, 64, backend, 8)
    assert (gc == oc).all() and (gk == ok).all() and (gd.view(np.uint32) == od.view(np.uint32)).all()
    assert st["n_dist_evals"] == int(ost[:, 0].sum())
    # (b) the stored-vector twin: materialised embeddings, same construction -> same graph, same neighbours
    dE = la.DeviceArray((n, d), np.float32)
    chk(Lc.leann_recompute_encode_device(r, 0, n, dE.ptr, None))
    la.sync()
    s2 = la.BackendSearcher.build_device(backend, dE.ptr, n, d, d, deg, 64)
    g2 = s2.graph_export()
    assert (g2["adj0"] == g["adj0"]).all()
    k2, d2, _ = s2.search_batch(Q, k, 64)
    print(f"recompute-on vs stored twin (backend {backend}, h = {h}): max |dist diff| = {np.abs(d2 - gd).max():.3e}, equal keys {(k2 == gk).mean():.4f}")
    assert np.abs(d2 - gd).max() <= 1e-5
    assert (k2 == gk).mean() >= 0.99  # identical except across float near-ties
    s2.close()
    s.close()
    Lc.leann_recompute_close(r)


def test_wide_recompute_on_graph_round_trips_through_its_file(la, po, gpu, tmp_path):
    n, d, nq, k, h = GRAPH_N, GRAPH_D, GRAPH_NQ, GRAPH_K, 256
    Lc, chk = la.lib(), la._native.check
    F, W, Q, r, keep = _graph_setup(la, po, h)
    hb = C.c_void_p()
    chk(Lc.leann_recompute_build_index(r, 0, 16, 64, C.byref(hb)))
    s = la.BackendSearcher(hb, 0)
    stem = str(tmp_path / "documents.leann")
    s.save(stem)
    g = s.graph_export()
    size = (tmp_path / "documents.index").stat().st_size
    assert size == 128 + n + 4 * n + 4 * n * g["M0"] + 4 * g["n_upper_lists"] * g["M"] + n * 520 + 4 * h * d  # W as f32 [feat_h x dims]
    s2 = la.BackendSearcher.load(0, stem, d)
    g2 = s2.graph_export()
    assert g2["dims"] == 1536 and g2["n"] == n
    for key in ("levels", "upper_off", "adj0", "adjU"):
        assert (g[key] == g2[key]).all(), key
    rows1, rows2 = np.zeros((n, 520), np.uint8), np.zeros((n, 520), np.uint8)
    chk(Lc.leann_backend_feature_rows_export(s._h, None, None, rows1.ctypes.data))
    chk(Lc.leann_backend_feature_rows_export(s2._h, None, None, rows2.ctypes.data))
    assert (rows1 == rows2).all()
    k1, d1, c1 = s.search_batch(Q, k, 64)
    k2, d2, c2 = s2.search_batch(Q, k, 64)
    assert (k1 == k2).all() and (d1.view(np.uint32) == d2.view(np.uint32)).all() and (c1 == c2).all()
    s2.close()
    s.close()
    Lc.leann_recompute_close(r)


TOPICS = ["rust ownership borrow checker lifetimes", "python asyncio event loop coroutine", "vector database embedding search",
          "graph traversal beam hnsw neighbours", "gpu kernel wavefront lds bandwidth", "bm25 ranking term frequency"]


def test_wide_cli_recompute_graph_directory(la, gpu, tmp_path):
    """`leann build --recompute-graph --dimensions 1024` and `leann search` on the result against the stored-vector twin of the same
    provider, as test_pruned_directory_with_recompute_graph_is_walked asserts at 384.
    File sizes with 600 passages, HNSW M = 16: per passage 1 (level) + 4 (offset) + 128 (level-0 list) + 520 (features + norm) =
    653 B against 133 + 4 096 = 4 229 B for the twin, plus — once — 256 x 1024 f32 weights = 1 048 576 B.  At 600 passages the
    one-off weights are 73 % of the recompute-graph file (0.39 MB + 1.05 MB against 2.54 MB: ratio 0.57), so the 0.3 the per-passage
    figures give (653 / 4 229 = 0.15) is asserted on the file without its weights and the whole file is held to 0.6."""
    n = 600
    docs = [dict(id=str(i + 1), text=f"passage {i} about {TOPICS[i % 6]} number {i * 7919 % 1000}", metadata=dict(lines=i)) for i in range(n)]
    (tmp_path / "docs.jsonl").write_text("\n".join(json.dumps(x) for x in docs))

    def run(*a):
        return subprocess.run([EXE, *a], capture_output=True, text=True)
    r = run("build", "--index-dir", str(tmp_path / "rg"), "--passages-jsonl", str(tmp_path / "docs.jsonl"), "--dimensions", "1024",
            "--graph-degree", "16", "--recompute-graph")
    assert r.returncode == 0, r.stderr
    r = run("build", "--index-dir", str(tmp_path / "full"), "--passages-jsonl", str(tmp_path / "docs.jsonl"), "--dimensions", "1024",
            "--graph-degree", "16", "--embedding-mode", "synthetic-linear")
    assert r.returncode == 0, r.stderr
    files = set(os.listdir(tmp_path / "rg"))
    assert "documents.index" in files and "documents.embeddings" not in files
    meta = json.loads((tmp_path / "rg" / "documents.leann.meta.json").read_text())
    assert meta["is_pruned"] and meta["is_recompute"] and meta["embedding_mode"] == "synthetic-linear" and meta["dimensions"] == 1024
    sz_rg, sz_full = os.path.getsize(tmp_path / "rg" / "documents.index"), os.path.getsize(tmp_path / "full" / "documents.index")
    weights = 4 * 256 * 1024
    print(f"index file: recompute-graph {sz_rg} B (weights {weights} B), stored-vector twin {sz_full} B")
    assert sz_rg - weights < 0.3 * sz_full
    assert sz_rg < 0.6 * sz_full
    for q in ("gpu kernel wavefront lds bandwidth for the win", "what about rust ownership and the borrow checker"):
        a = json.loads(run("search", q, "-i", str(tmp_path / "rg"), "--top-k", "6", "--format", "json", "--complexity", "128").stdout)
        b = json.loads(run("search", q, "-i", str(tmp_path / "full"), "--top-k", "6", "--format", "json", "--complexity", "128").stdout)
        assert len(a) == 6 and [x["score"] for x in a] == sorted(x["score"] for x in a)  # distances, ascending: a graph walk
        assert np.allclose([x["score"] for x in a], [x["score"] for x in b], atol=1e-5)
        assert len({x["id"] for x in a} & {x["id"] for x in b}) >= 5
