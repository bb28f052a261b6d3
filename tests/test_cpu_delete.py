"""CPU suite: removals — argument validation, the tombstone sidecar's writer and validator, and self-checks of the numpy
restatement of delete consolidation (tests/consolidate_ref.py).  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import consolidate_ref as cr
import delete_cases as dc


def _err(la):
    return la.lib().leann_last_error().decode()


def test_null_arguments(la):
    L = la.lib()
    keys = np.array([1, 2], np.uint64)
    n = C.c_size_t(7)
    assert L.leann_backend_remove(None, keys.ctypes.data_as(la._native.u64p), 2, C.byref(n)) == 1
    assert "null" in _err(la) and n.value == 0
    assert L.leann_backend_consolidate(None) == 1 and "null" in _err(la)
    assert L.leann_backend_live_len(None) == 0
    assert L.leann_backend_removed_bitmap(None, None, None) == 1
    assert L.leann_backend_remove_from_index(0, None, 3, 8, b"x.leann") == 1
    assert L.leann_backend_remove_from_index(0, keys.ctypes.data_as(la._native.u64p), 2, 8, None) == 1


def test_remove_from_a_missing_index_names_the_file(la, tmp_path):
    keys = np.array([1], np.uint64)
    stem = str(tmp_path / "documents.leann")
    rc = la.lib().leann_backend_remove_from_index(0, keys.ctypes.data_as(la._native.u64p), 1, 8, stem.encode())
    assert rc == 2 and "documents.index" in _err(la)


def _write(la, path, bits, pending=0):
    bm = np.packbits(bits, bitorder="little")
    return la.lib().leann_tombstones_write(str(path).encode(), bm.ctypes.data_as(la._native.u8p), len(bits), pending), bm


def _read(la, path, n):
    bm = np.zeros((n + 7) // 8, np.uint8)
    cnt, pend = C.c_uint64(0), C.c_uint64(0)
    rc = la.lib().leann_tombstones_read(str(path).encode(), n, bm.ctypes.data_as(la._native.u8p), C.byref(cnt), C.byref(pend))
    return rc, bm, cnt.value, pend.value


@pytest.mark.parametrize("n", [1, 8, 61, 4096, 4099])
def test_sidecar_round_trip(la, tmp_path, n):
    rng = np.random.default_rng(n)
    bits = rng.random(n) < 0.3
    bits[0] = True
    path = tmp_path / "documents.tombstones"
    rc, bm = _write(la, path, bits, pending=1)
    assert rc == 0
    raw = open(path, "rb").read()
    assert raw[:8] == b"LEANNTB1" and len(raw) == 32 + (n + 7) // 8
    assert [int.from_bytes(raw[8 + 8 * i: 16 + 8 * i], "little") for i in range(3)] == [n, int(bits.sum()), 1]
    rc, got, cnt, pend = _read(la, path, n)
    assert rc == 0 and (got == bm).all() and cnt == int(bits.sum()) and pend == 1


def test_sidecar_validation(la, tmp_path):
    n = 61
    bits = np.zeros(n, bool)
    bits[[0, 17, 60]] = True
    path = tmp_path / "documents.tombstones"
    assert _write(la, path, bits)[0] == 0
    raw = open(path, "rb").read()

    def refused(data, n_expected=n):
        open(path, "wb").write(data)
        rc = _read(la, path, n_expected)[0]
        return rc, _err(la)

    assert refused(raw[:-1])[0] == 3                                            # truncated
    assert refused(raw + b"\0")[0] == 3                                         # too long
    rc, msg = refused(raw[:16] + (4).to_bytes(8, "little") + raw[24:])          # wrong popcount
    assert rc == 3 and "count" in msg
    assert refused(raw[:-1] + bytes([raw[-1] | 0x80]))[0] == 3                  # a padding bit (and the popcount) off
    padded = raw[:16] + (4).to_bytes(8, "little") + raw[24:-1] + bytes([raw[-1] | 0x20])
    rc, msg = refused(padded)                                                   # popcount consistent, padding bit 61 set
    assert rc == 3 and "padding" in msg
    assert refused(b"LEANNTBX" + raw[8:])[0] == 3                               # magic
    assert refused(raw, n_expected=62)[0] == 3                                  # made for another row count
    assert refused(raw[:24] + (9).to_bytes(8, "little") + raw[32:])[0] == 3     # more pending than removed
    assert refused(raw)[0] == 0
    assert _read(la, tmp_path / "absent.tombstones", n)[0] == 2
    # the writer refuses bits past n
    bm = np.array([0xFF], np.uint8)
    assert la.lib().leann_tombstones_write(str(path).encode(), bm.ctypes.data_as(la._native.u8p), 5, 0) == 1


@pytest.mark.parametrize("kind,M,M0,max_level", [("hnsw", 4, 8, 2), ("diskann", 6, 6, 0)])
def test_reference_self_checks(kind, M, M0, max_level):
    rng = np.random.default_rng(64)
    n = 64
    g = cr.random_graph(rng, kind, n, 16, M, M0, max_level)
    removed = rng.random(n) < 0.3
    removed[g["entry"]] = True
    assert cr.pending(g, removed) > 0
    for two_stage in (True, False):
        out = cr.consolidate(g, removed, two_stage=two_stage)
        assert cr.pending(out, removed) == 0
        assert not removed[out["entry"]] and g["levels"][out["entry"]] == out["max_level"]
        for adj, old in ((out["adj0"], g["adj0"]), (out["adjU"], g["adjU"])):
            for row, (l, lo) in enumerate(zip(adj, old)):
                ids = l[l != cr.EMPTY]
                assert len(set(ids.tolist())) == len(ids)                        # no duplicates
                assert (l[len(ids):] == cr.EMPTY).all()                          # compact
                loi = lo[lo != cr.EMPTY]
                if not removed[loi].any() and len(ids):                          # named nothing removed: untouched (or cleared)
                    assert (l == lo).all()
        live = np.flatnonzero(~removed)
        l0 = out["adj0"][live]
        assert not removed[l0[l0 != cr.EMPTY]].any() and (l0 != live[:, None]).all()
        assert (out["adj0"][removed] == cr.EMPTY).all()
    # nothing removed: nothing changes
    same = cr.consolidate(g, np.zeros(n, bool))
    assert (same["adj0"] == g["adj0"]).all() and (same["adjU"] == g["adjU"]).all() and same["entry"] == g["entry"]


def test_reference_prune_rules():
    # dist = 1 - dot.  c0 is nearest to p; c1 is closer to c0 (0.375) than to p (0.75): occluded; c2 is at distance 1 from both
    X = np.array([[1, 0, 0], [0.5, 0.5, 0], [0.25, 1, 0], [0, 0, 1]], np.float32)
    cid = np.array([1, 2, 3])
    cd = (np.float32(1) - X[cid] @ X[0]).astype(np.float32)
    assert cd.tolist() == [0.5, 0.75, 1.0]
    assert cr.prune(X, cid, cd, 3, 0.0, True) == [0, 2]      # HNSW: dist(c2, c0) = 1 is not < dist(c2, p) = 1
    assert cr.prune(X, cid, cd, 1, 0.0, True) == [0]
    assert cr.prune(X, cid, cd, 3, 1.2, False) == [0, 2]     # Vamana, one stage: 1.2 * 1 <= 1 fails, c2 stays
    # two stages: the first walk (alpha = 1) drops c2 (1 <= 1); the relaxed second walk takes it back
    assert cr.prune(X, cid, cd, 3, 1.2, True) == [0, 2]
    assert cr.prune(X, cid, cd, 3, 1.0, True) == [0]         # alpha = 1: one stage by definition


# ---- the cases of tests/test_gpu_delete_edges.py, on the reference alone ------------------------------------------------------

def test_sparse_rows_keep_the_exactness_argument():
    rng = np.random.default_rng(1)
    for rows, nnz in (("sparse", 3), ("mixed", 8), ("dense", 0)):
        X = cr.random_graph(rng, "diskann", 64, 4096, 4, 4, 0, rows=rows, nnz=nnz)["X"]
        assert X.dtype == np.float32 and (X * 8 == np.round(X * 8)).all() and np.abs(X).max() <= 0.25
        if rows == "sparse":
            assert ((X != 0).sum(axis=1) == nnz).all()
        if rows == "mixed":
            assert ((X[1::2] != 0).sum(axis=1) == nnz).all() and ((X[0::2] != 0).sum(axis=1) > 2000).all()
        # |dot| <= 4096 / 16 = 256 in multiples of 1/64: 2^14 steps, exact in f32 whatever the order of the sum
        assert (np.abs(X.astype(np.float64) @ X.astype(np.float64).T) <= 256).all()
    # the dense recipe draws what it always drew: graphs of the older tests keep their bytes
    a = cr.random_graph(np.random.default_rng(7), "hnsw", 64, 16, 4, 8, 2)
    b = cr.random_graph(np.random.default_rng(7), "hnsw", 64, 16, 4, 8, 2, rows="dense", nnz=5)
    assert (a["X"] == b["X"]).all() and (a["adj0"] == b["adj0"]).all() and (a["adjU"] == b["adjU"]).all()
    assert (a["X"] == (np.random.default_rng(7).integers(-2, 3, (64, 16)) / 8.0).astype(np.float32)).all()


@pytest.mark.parametrize("name", list(dc.CASES))
def test_case_reaches_the_branch_it_is_there_for(name):
    c = dc.CASES[name]
    g, removed, special = dc.graph(name)
    want = dc.reference(name)
    dc.check_needs(name, want)
    cn = want["counters"]
    assert c["n"] % 8 and c["n"] % 256 and removed[g["entry"]] and not removed[want["entry"]]
    assert cr.pool_size(g) == (256 if max(c["M"], c["M0"]) > 64 else 128)
    assert cr.pending(g, removed) > 0 and cr.pending(want, removed) == 0
    assert cn["repairs"] == sum(cn[k] for k in ("pools_0", "pools_1", "pools_2_32", "pools_33_64", "pools_65_128", "pools_129_255")) + \
        (cn["pools_eq_nc"] if cr.pool_size(g) == 256 else 0)
    l0 = g["adj0"]
    clean = ~removed & ~(removed[np.where(l0 == cr.EMPTY, 0, l0)] & (l0 != cr.EMPTY)).any(axis=1)
    assert clean.sum() >= 8 and (want["adj0"][clean] == l0[clean]).all()
    lens = (want["adj0"][~removed & ~clean] != cr.EMPTY).sum(axis=1)     # every other live level-0 list was repaired
    assert cn["lists_gt64"] >= int((lens > 64).sum()) and want["counters_by_level"][0]["lists_full"] == int((lens == c["M0"]).sum())
    if "full_dead" in special:                                   # width + 1 sources: width * (width + 1) slots
        l = l0[special["full_dead"]]
        assert (l != cr.EMPTY).all() and removed[l].all() and len(set(l.tolist())) == c["M0"] == 128
        assert (c["M0"] + 1) * c["M0"] == 16512 and -(-16512 // 256) == 65
    if "empty_pool" in special:
        assert (want["adj0"][special["empty_pool"]] == cr.EMPTY).all()


def test_reference_states():
    """the states of test_gpu_delete_edges.py as the reference sees them"""
    rng = np.random.default_rng(23)
    g = cr.random_graph(rng, "hnsw", 515, 40, 8, 16, 2)
    everything = cr.consolidate(g, np.ones(515, bool))
    assert (everything["adj0"] == cr.EMPTY).all() and (everything["adjU"] == cr.EMPTY).all()
    assert everything["entry"] == g["entry"] and everything["max_level"] == g["max_level"] and everything["counters"]["repairs"] == 0
    removed = g["levels"] >= 1
    flat = cr.consolidate(g, removed)
    assert flat["max_level"] == 0 and flat["entry"] == np.flatnonzero(~removed)[0] and (flat["adjU"] == cr.EMPTY).all()
    assert flat["counters_by_level"][1]["repairs"] == 0 and flat["counters_by_level"][0]["repairs"] > 0
    # a second round on a repaired graph: the repaired lists are the old lists of the next pass
    first = rng.random(515) < 0.25
    one = cr.consolidate(g, first)
    second = first | (rng.random(515) < 0.15)
    two = cr.consolidate(one, second)
    assert cr.pending(one, second) > 0 and cr.pending(two, second) == 0
    assert (two["adj0"] != cr.consolidate(g, second)["adj0"]).any()    # not the same as removing everything at once


@pytest.mark.parametrize("alpha,two_stage", [(0.0, True), (1.2, False), (1.2, True)])
def test_reference_prune_matches_the_oracle_past_64_kept(po, alpha, two_stage):
    """cr.prune against the C oracle's prune on one wide pool: 256 candidates, limit 128, rows sparse enough that more than 64 are
    kept and one dense row so that every rule drops some — the numpy rule is then not the only statement of that path"""
    rng = np.random.default_rng(256)
    X = cr.sparse_rows(rng, 300, 256, 3)
    X[7] = (rng.integers(-2, 3, 256) / 8.0).astype(np.float32)
    ids = np.concatenate([[7], rng.choice(np.arange(8, 300), 255, replace=False)])
    d = (np.float32(1.0) - (X[ids].astype(np.float64) @ X[0].astype(np.float64)).astype(np.float32)).astype(np.float32)
    o = np.lexsort((ids, d))
    ids, d = ids[o], d[o]
    want = po.prune(X, ids, d, 128, alpha, two_stage).tolist()
    info = {}
    got = list(cr.prune(X, ids.astype(np.int64), d, 128, alpha, two_stage, info))
    assert got == want and 64 < len(got) <= 128
    # the rule dropped something on the way (one-stage alpha = 1.2 needs a dot of 1/6 to drop: rows of three 1/8ths hardly have one)
    assert got != list(range(len(got))) or (alpha > 1 and not two_stage)
    assert (info["second_stage"] > 0) == (two_stage and alpha > 1)
    assert len(cr.prune(X, ids.astype(np.int64), d, 64, alpha, two_stage)) == 64
