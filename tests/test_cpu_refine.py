"""CPU suite: refining results on exact rows (include/leann_backend.h, csrc/refine.hip) — what needs no GPU.  Every new entry point
refuses bad arguments with LEANN_ERR_INVALID and a message naming the argument before any device work, and the numpy restatement the
GPU tests compare against (tests/refine_ref.py) agrees with the oracle's own f32 search."""
import ctypes as C

import numpy as np

import refine_ref
from util import synth

INVALID, NOT_FOUND, FORMAT = 1, 2, 3


def _err(L):
    return L.leann_last_error().decode()


def test_new_entry_points_reject_bad_arguments_without_a_gpu(la, tmp_path):
    L = la.lib()
    blocks = L.leann_debug_device_blocks()
    out = C.c_void_p()
    X = np.zeros((4, 8), np.float32)
    xp = X.ctypes.data_as(C.POINTER(C.c_float))
    fake = C.c_void_p(0x1000)  # never dereferenced: every call below is refused first

    # ---- the rows
    assert L.leann_exact_rows_from_device(None, 4, 8, 8, 0, 0, C.byref(out)) == INVALID and "d_rows" in _err(L) and not out.value
    assert L.leann_exact_rows_from_device(fake, 4, 8, 8, 0, 0, None) == INVALID and "out" in _err(L)
    assert L.leann_exact_rows_from_device(fake, 4, 8, 6, 0, 0, C.byref(out)) == INVALID and "ld = 6" in _err(L)
    assert L.leann_exact_rows_from_device(fake, 4, 8, 4, 0, 0, C.byref(out)) == INVALID and "ld = 4" in _err(L)
    assert L.leann_exact_rows_from_device(fake, 4, 0, 8, 0, 0, C.byref(out)) == INVALID and "dims = 0" in _err(L)
    assert L.leann_exact_rows_from_device(fake, 4, 4097, 4100, 0, 0, C.byref(out)) == INVALID and "dims = 4097" in _err(L)
    assert L.leann_exact_rows_from_device(fake, 2 ** 32 - 1, 8, 8, 0, 0, C.byref(out)) == INVALID and "n = " in _err(L)
    assert L.leann_exact_rows_from_host(None, 4, 8, 0, 0, 0, C.byref(out)) == INVALID and "null rows" in _err(L)
    assert L.leann_exact_rows_from_host(xp, 4, 8, 0, 0, 2, C.byref(out)) == INVALID and "placement = 2" in _err(L)
    assert L.leann_exact_rows_from_host(xp, 4, 8, 0, 0, -1, C.byref(out)) == INVALID and "placement = -1" in _err(L)
    assert L.leann_exact_rows_from_host(xp, 4, 5000, 0, 0, 1, C.byref(out)) == INVALID and "dims = 5000" in _err(L)
    assert L.leann_exact_rows_from_host(xp, 4, 8, 0, 0, 0, None) == INVALID and "out" in _err(L)
    assert L.leann_exact_rows_open(None, 8, 0, 0, 0, C.byref(out)) == INVALID and "embeddings_path" in _err(L)
    assert L.leann_exact_rows_open(b"x.embeddings", 8, 0, 0, 3, C.byref(out)) == INVALID and "placement = 3" in _err(L)
    assert L.leann_exact_rows_open(b"x.embeddings", 0, 0, 0, 0, C.byref(out)) == INVALID and "dims = 0" in _err(L)
    missing = str(tmp_path / "documents.embeddings").encode()
    for placement in (0, 1):
        assert L.leann_exact_rows_open(missing, 8, 0, 0, placement, C.byref(out)) == NOT_FOUND
        assert "leann build --recompute" in _err(L) and "documents.embeddings" in _err(L) and not out.value
    (tmp_path / "documents.embeddings").write_bytes(b"\0" * 100)  # not a whole number of 8-float rows
    assert L.leann_exact_rows_open(missing, 8, 0, 0, 1, C.byref(out)) == FORMAT and "whole number" in _err(L)
    assert L.leann_exact_rows_len(None) == 0 and L.leann_exact_rows_placement(None) == -1
    L.leann_exact_rows_close(None)
    if la.device_count() == 0:  # only the missing GPU stands in the way: never a copy kept on the CPU
        assert L.leann_exact_rows_from_host(xp, 4, 8, 0, 0, 1, C.byref(out)) == 4 and "no CPU fallback" in _err(L)

    # ---- the rerank, on borrowed rows (an object that owns nothing and touches no device until a kernel is launched)
    assert L.leann_exact_rows_from_device(fake, 4, 8, 8, 0, 100, C.byref(out)) == 0 and out.value
    rows = out
    assert L.leann_exact_rows_len(rows) == 4 and L.leann_exact_rows_placement(rows) == 0
    assert L.leann_rerank_batch_device(None, fake, 1, fake, fake, 4, 2, fake, fake, fake, None, None) == INVALID and "null rows" in _err(L)
    for i, name in ((1, "d_queries"), (3, "d_keys"), (4, "d_counts"), (7, "d_out_keys"), (8, "d_out_dists"), (9, "d_out_counts")):
        args = [rows, fake, 1, fake, fake, 4, 2, fake, fake, fake, None, None]
        args[i] = None
        assert L.leann_rerank_batch_device(*args) == INVALID and name in _err(L)
    assert L.leann_rerank_batch_device(rows, fake, 1, fake, fake, 4, 0, fake, fake, fake, None, None) == INVALID and "top_k = 0" in _err(L)
    assert L.leann_rerank_batch_device(rows, fake, 1, fake, fake, 4, 5, fake, fake, fake, None, None) == INVALID
    assert "top_k = 5" in _err(L) and "fetch_k = 4" in _err(L)
    assert L.leann_rerank_batch_device(rows, fake, 1, fake, fake, 1025, 5, fake, fake, fake, None, None) == INVALID and "fetch_k = 1025" in _err(L)
    assert L.leann_rerank_batch_device(rows, fake, 0, None, None, 4, 2, None, None, None, None, None) == 0  # nothing to do, nothing touched

    # ---- walk + rerank
    q = np.zeros(8, np.float32)
    keys, dists, cnt = np.zeros(4, np.uint64), np.zeros(4, np.float32), np.zeros(1, np.uint32)
    f32p, u64p, u32p = (C.POINTER(t) for t in (C.c_float, C.c_uint64, C.c_uint32))
    assert L.leann_backend_search_refined_batch_device(None, rows, fake, 1, 2, 4, 16, None, 0, fake, fake, fake, None, None) == INVALID
    assert "null handle" in _err(L)
    assert L.leann_backend_search_refined_batch(None, rows, q.ctypes.data_as(f32p), 1, 2, 4, 16, None, 0, keys.ctypes.data_as(u64p),
                                                dists.ctypes.data_as(f32p), cnt.ctypes.data_as(u32p), None) == INVALID
    assert "null handle" in _err(L)
    L.leann_exact_rows_close(rows)
    assert L.leann_debug_device_blocks() == blocks  # refused calls and borrowed rows own nothing

    # ---- the Python layer: an unknown placement is refused by name, a missing file by the library
    import pytest
    with pytest.raises(la.LeannError) as e:
        la.ExactRows.from_host(X, placement="disk")
    assert e.value.code == INVALID and "placement" in str(e.value)
    with pytest.raises(la.LeannError) as e:
        la.ExactRows.open(tmp_path / "nothing.embeddings", 8, placement="host")
    assert e.value.code == NOT_FOUND and "--recompute" in str(e.value)


def test_restatement_agrees_with_the_oracle(po):
    """300 x 96: the oracle's own f32 search result, refined on the rows it walked, comes back unchanged — keys, distance bits and
    counts — and refining the walk's 20 best gives the walk's 10 best (same beam, so the 10 best are a prefix)."""
    n, d, k, ef = 300, 96, 10, 48
    X, Q = synth(po, n, d), synth(po, 40, d, stream=1)
    G = po.Graph.build_hnsw(X, M=8, efc=48)
    gk, gd, gc, _ = G.search_batch(Q, k, ef)
    assert (gc == k).all()
    rk, rd, rc, sk = refine_ref.rerank(po, X, Q, gk, gc, k)
    assert (rk == gk).all() and (rd.view(np.uint32) == gd.view(np.uint32)).all() and (rc == gc).all() and (sk == 0).all()
    wk, _, wc, _ = G.search_batch(Q, 20, ef)
    rk, rd, rc, _ = refine_ref.rerank(po, X, Q, wk, wc, k)
    assert (rk == gk).all() and (rd.view(np.uint32) == gd.view(np.uint32)).all() and (rc == k).all()
    # a key offset moves keys, not rows; out-of-range keys and the tail value are skipped and counted; a duplicate comes back twice
    lst = np.array([[1007, 5, 1003, 1003, refine_ref.NO_KEY, 1300, 1299, 999]], np.uint64)
    rk, rd, rc, sk = refine_ref.rerank(po, X, Q[:1], lst, np.array([7], np.uint32), 8, key_offset=1000)
    assert rc[0] == 4 and sk[0] == 3 and sorted(rk[0, :4].tolist()) == [1003, 1003, 1007, 1299]
    assert (rk[0, 4:] == refine_ref.NO_KEY).all() and np.isinf(rd[0, 4:]).all()
    assert (np.diff(refine_ref.orderable(rd[0, :4]).astype(np.int64)) >= 0).all()
    assert rd[0, list(rk[0, :4]).index(1007)] == po.dist_canon(Q[0], X[7])
