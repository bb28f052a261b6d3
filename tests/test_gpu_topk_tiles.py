"""-m gpu: the recompute search's query-tile loop together with candidate emission.  The feature-stationary kernel takes 256 queries per
pass over the passages; the other suites' largest batch is 150, so none of them runs a second tile through the emission schedule
(csrc/topk_plan.h), where each tile has its own rows of `best` and `candA` (select_chunk's q0) but shares the threshold slots, the
candidate lists and the overflow word.  h = 256, d = 128 (the smallest width the kernel takes), k = 10; n = 20000 cuts chunks
(0, 16384) and (16384, 3616), nq = 257 leaves a second tile of one query.  Every answer must equal the slab schedule's
(LEANN_DEBUG_NO_EMIT=1: same kernel arithmetic) bit for bit; scores of queries 0, 255 and 256 are held to the oracle restatement on
the winners within 1e-5, the bound test_gpu_recompute.py uses for that comparison."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = 0x5EED0001
H, D, K, NQ = 256, 128, 10, 257


def _search(la, r, dQ, dM=None):
    L, chk = la.lib(), la._native.check
    dk, ds, dc = la.DeviceArray((NQ, K), np.uint64), la.DeviceArray((NQ, K), np.float32), la.DeviceArray(NQ, np.uint32)
    chk(L.leann_recompute_search_batch_device(r, dQ.ptr, NQ, K, dM.ptr if dM is not None else None, dk.ptr, ds.ptr, dc.ptr, None))
    la.sync()
    return dk.to_host(), ds.to_host(), dc.to_host()


def _both_schedules(la, monkeypatch, r, dQ, dM=None):
    """the answer on the default schedule, after holding it bit for bit to the slab schedule's"""
    gk, gs, gc = _search(la, r, dQ, dM)
    monkeypatch.setenv("LEANN_DEBUG_NO_EMIT", "1")
    la.lib().leann_debug_reload_env()
    sk, ss, sc = _search(la, r, dQ, dM)
    monkeypatch.delenv("LEANN_DEBUG_NO_EMIT")
    la.lib().leann_debug_reload_env()
    assert (gc == sc).all() and (gk == sk).all() and (gs.view(np.uint32) == ss.view(np.uint32)).all()
    return gk, gs, gc


@pytest.fixture(scope="module")
def two_tiles(la, po, gpu):
    n = 20000
    F, W = po.synth_features(SEED, H, 64, 1.0, 0, 0, n), po.synth_weights(SEED, H, D)
    Q = po.recompute_encode(po.synth_features(SEED, H, 64, 1.0, 1, 0, NQ), W)
    keep = la.DeviceArray.from_host(F), la.DeviceArray.from_host(W), la.DeviceArray.from_host(Q)
    r = C.c_void_p()
    la._native.check(la.lib().leann_recompute_create(keep[0].ptr, n, H, keep[1].ptr, D, 0, 0, C.byref(r)))
    yield n, F, W, Q, r, keep
    la.lib().leann_recompute_close(r)


def _hold_winners_to_oracle(po, F, W, Q, gk, gs):
    for i in (0, 255, 256):
        E = po.recompute_encode(F[gk[i].astype(np.int64)], W)
        assert np.abs(E @ Q[i] - gs[i]).max() <= 1e-5


def test_two_tiles_with_emission(la, po, two_tiles, monkeypatch):
    n, F, W, Q, r, keep = two_tiles
    gk, gs, gc = _both_schedules(la, monkeypatch, r, keep[2])
    assert (gc == K).all() and (np.diff(gs, axis=1) <= 0).all() and (gk < n).all()
    _hold_winners_to_oracle(po, F, W, Q, gk, gs)


@pytest.mark.parametrize("no_list", [False, True])
def test_two_tiles_with_emission_and_allow_mask(la, po, two_tiles, monkeypatch, no_list):
    """Every fifth position allowed.  As called, the early filter compacts the 4000 allowed positions into a row list, which is one
    slab chunk; LEANN_RECOMPUTE_NO_LIST=1 keeps the masked pass over all rows, so the mask goes through the emitted chunk too."""
    n, F, W, Q, r, keep = two_tiles
    if no_list:
        monkeypatch.setenv("LEANN_RECOMPUTE_NO_LIST", "1")
        la.lib().leann_debug_reload_env()
    idx = np.arange(0, n, 5)
    mask = np.zeros((n + 7) // 8, np.uint8)
    np.bitwise_or.at(mask, idx >> 3, (1 << (idx & 7)).astype(np.uint8))
    dM = la.DeviceArray.from_host(mask)
    gk, gs, gc = _both_schedules(la, monkeypatch, r, keep[2], dM)
    assert (gc == K).all() and (gk % 5 == 0).all() and (gk < n).all()
    _hold_winners_to_oracle(po, F, W, Q, gk, gs)


def test_overflow_in_one_tile_only(la, po, gpu, monkeypatch):
    """Features interpolated from u to v as in test_candidate_list_overflow_falls_back, at n = 32768: chunks (0, 16384) and
    (16384, 16384).  Query 256, alone in the second tile, is the embedding of v: its score rises with the position, every row of
    the emitted chunk reaches its 10th best of the first and its list of 8192 keys overflows.  Queries 0..255 are embeddings of
    features scattered around u: their scores fall along the way and their lists stay short.  Both facts are asserted on the host
    before the run (with 2e-5 to spare against the oracle's scores), so the overflow, and that it is the second tile's alone, is
    certain and not hoped for.  The search must notice and repeat on the slab schedule for the whole batch: same answer."""
    n, cap = 32768, 8192
    L, chk = la.lib(), la._native.check

    def bf16(x):
        return ((np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) + 0x8000) >> 16).astype(np.uint16)  # round half up is fine here

    rng = np.random.default_rng(1)
    W = po.synth_weights(SEED, H, D)
    u, v = rng.standard_normal(H).astype(np.float32), rng.standard_normal(H).astype(np.float32)
    t = (np.arange(n, dtype=np.float32) / n)[:, None]
    F = bf16((1 - t) * u[None, :] + t * v[None, :])
    qf = np.concatenate([bf16(u[None, :] + 0.25 * rng.standard_normal((NQ - 1, H)).astype(np.float32)), bf16(v[None, :])])
    Q = po.recompute_encode(qf, W)
    S = po.recompute_encode(F, W) @ Q.T                                     # [n x NQ] oracle scores
    kth = np.sort(S[:16384], axis=0)[-K]                                    # each query's 10th best of the first chunk
    assert (S[16384:, 256] >= kth[256] + 2e-5).sum() > cap
    assert ((S[16384:, :256] >= kth[None, :256] - 2e-5).sum(axis=0) < cap).all()
    dF, dW, dQ = la.DeviceArray.from_host(F), la.DeviceArray.from_host(W), la.DeviceArray.from_host(Q)
    r = C.c_void_p()
    chk(L.leann_recompute_create(dF.ptr, n, H, dW.ptr, D, 0, 0, C.byref(r)))
    gk, gs, gc = _both_schedules(la, monkeypatch, r, dQ)
    assert (gc == K).all() and gk[256].min() > n - 2000                     # query 256's winners are at the far end
    L.leann_recompute_close(r)
