"""-m gpu: wide graphs — lists of up to 128 ids (HNSW graph_degree <= 64, level 0 holds 2 M; DiskANN R <= 128).
The traversal kernel reads such a list two ids per lane (search.cuh, LW = 2), the builder prunes 256-candidate pools (build.hip,
NCWIDE).  Bars: the kernel against the oracle walk bit for bit (ids, distance bits, all three visit counters) on oracle-built graphs,
so the kernel is isolated from the builder; the GPU-built wide graphs are valid, as good as the sequential builder's, and searched
exactly like their export; narrow builds are byte-identical to the graphs recorded before the wide builder existed."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from util import SEED, recall_at_k, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = 0xFFFFFFFF


def _assert_same(G, s, Q, k, ef, algo=0):  # algo 1: the oracle's sorted-list GreedySearch (Vamana)
    ok, od, oc, ost = G.search_batch(Q, k, ef, algo, nthreads=8)
    s.stats(reset=True)
    gk, gd, gc = s.search_batch(Q, k, ef)
    st = s.stats()
    assert (gc == oc).all()
    assert (gk == ok).all(), f"ids differ in {(gk != ok).any(axis=1).sum()} of {len(Q)} queries"
    assert (gd.view(np.uint32) == od.view(np.uint32)).all()
    assert st["n_dist_evals"] == int(ost[:, 0].sum())
    assert st["n_hops_base"] == int(ost[:, 1].sum())
    assert st["n_hops_upper"] == int(ost[:, 2].sum())
    return gk


def _assert_same_filtered(G, s, Q, k, ef, bm, algo=0):
    ok, od, oc, _ = G.search_filtered_batch(Q, k, ef, bm, algo, nthreads=8)
    gk, gd, gc = s.search_filtered_batch(Q, k, ef, bm)
    assert (gc == oc).all() and (gk == ok).all() and (gd.view(np.uint32) == od.view(np.uint32)).all()


def _wide_lists(adj0):
    return int(((np.asarray(adj0) != EMPTY).sum(1) > 64).sum())


def _knob(la, monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, str(value))
    la.lib().leann_debug_reload_env()


# ---- the traversal kernel on oracle-built graphs --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def queries(po):
    return {d: synth(po, 2048, d, stream=1) for d in (128, 768, 1536)}


@pytest.mark.parametrize("kind,deg,n,d", [("hnsw", 48, 3000, 128), ("hnsw", 64, 3000, 128), ("hnsw", 64, 3000, 768),
                                          ("hnsw", 48, 2000, 1536), ("hnsw", 64, 2000, 1536),
                                          ("vamana", 96, 3000, 128), ("vamana", 128, 3000, 128), ("vamana", 128, 2000, 768)])
def test_search_on_oracle_wide_graph_matches_oracle(la, po, gpu, queries, monkeypatch, kind, deg, n, d):
    X = synth(po, n, d)
    if kind == "hnsw":
        G = po.Graph.build_hnsw(X, M=deg, efc=128)
        lv, uo, a0, aU = G.export()
        s = la.BackendSearcher.from_arrays(la.BackendType.Hnsw, X, deg, 2 * deg, G.max_level, G.entry, lv, uo, a0, aU)
    else:
        G = po.Graph.build_vamana(X, R=deg, L=128)
        lv, uo, a0, aU = G.export()
        s = la.BackendSearcher.from_arrays(la.BackendType.DiskAnn, X, deg, deg, 0, G.entry, lv, uo, a0, np.zeros((0, deg), np.uint32))
    assert _wide_lists(a0) > 0  # the second half of a list (ids 64..127) is really walked
    Q = queries[d]
    algo = 0 if kind == "hnsw" else 1
    # batches of 1 and 64 (16 waves, latency form), 512 (8 waves), 2048 (4 waves, throughput form); ef below the degree and >= 128
    for nq, k, ef in ((1, 10, 64), (64, 10, 32), (64, 50, 160), (512, 10, 128), (2048, 10, 48), (2048, 1, 1)):
        _assert_same(G, s, Q[:nq], k, ef, algo)
    for nw in (4, 8, 16):  # every wave count on the same batch
        _knob(la, monkeypatch, "LEANN_DEBUG_NW", nw)
        _assert_same(G, s, Q[:256], 10, 96, algo)
    _knob(la, monkeypatch, "LEANN_DEBUG_NW", None)
    _knob(la, monkeypatch, "LEANN_DEBUG_HASH_BITS", 8)  # 256-slot LDS table: queries move to the HBM pool mid-search
    s.stats(reset=True)
    _assert_same(G, s, Q[:64], 10, 128, algo)
    _assert_same(G, s, Q[:1024], 10, 64, algo)
    _knob(la, monkeypatch, "LEANN_DEBUG_HASH_BITS", None)
    rng = np.random.default_rng(7)
    for sel in (0.10, 0.01):
        bm = np.packbits(rng.random(n) < sel, bitorder="little")
        _assert_same_filtered(G, s, Q[:64], 10, 128, bm, algo)
        _assert_same_filtered(G, s, Q[:1024], 10, 64, bm, algo)
    s.close()


@pytest.mark.parametrize("h,nq", [(256, 300), (256, 1024), (128, 300), (128, 1024)])
def test_recompute_on_graph_of_degree_64(la, po, gpu, h, nq):
    """graph with no stored vectors (bf16 feature rows, dist = 1 - <f, W q> / ||W^T f||) built at graph_degree 64 on the GPU: the
    search equals the oracle walk over the exported graph and feature rows bit for bit (h = 256: four rows per wave instruction)"""
    n, d, k, ef = 8000, 384, 10, 96
    Lc, chk = la.lib(), la._native.check
    F = po.synth_features(SEED, h, 64, 1.0, 0, 0, n)
    W = po.synth_weights(SEED, h, d)
    Q = po.recompute_encode(po.synth_features(SEED, h, 64, 1.0, 1, 0, nq), W)
    dF, dW = la.DeviceArray.from_host(F), la.DeviceArray.from_host(W)
    r = C.c_void_p()
    chk(Lc.leann_recompute_create(dF.ptr, n, h, dW.ptr, d, 0, 0, C.byref(r)))
    hb = C.c_void_p()
    chk(Lc.leann_recompute_build_index(r, 0, 64, 64, C.byref(hb)))
    s = la.BackendSearcher(hb, la.BackendType.Hnsw)
    fh, rb = C.c_uint32(0), C.c_uint32(0)
    chk(Lc.leann_backend_feature_rows_export(hb, C.byref(fh), C.byref(rb), None))
    rows = np.zeros((n, rb.value), np.uint8)
    chk(Lc.leann_backend_feature_rows_export(hb, None, None, rows.ctypes.data))
    g = s.graph_export()
    assert g["M0"] == 128 and _wide_lists(g["adj0"]) > 0
    s.stats(reset=True)
    gk, gd, gc = s.search_batch(Q, k, ef)
    st = s.stats()
    Gr = po.Graph.from_arrays(np.zeros((n, 1), np.float32), 64, 128, g["max_level"], g["entry"], g["levels"], g["upper_off"],
                              g["adj0"], g["adjU"])
    Gr.set_features(rows, fh.value, rb.value)
    ok, od, oc, ost = Gr.search_batch(po.project_queries(W, Q, fh.value), k, ef, 0, 8)
    assert (gc == oc).all() and (gk == ok).all() and (gd.view(np.uint32) == od.view(np.uint32)).all()
    assert st["n_dist_evals"] == int(ost[:, 0].sum())
    s.close()
    Lc.leann_recompute_close(r)


# ---- the GPU builder at wide degrees --------------------------------------------------------------------------------------------
def _rows(la, n, d, stream):
    buf = la.DeviceArray((n, d), np.float32)
    la._native.check(la.lib().leann_synth_rows_device(SEED, d, d, 64, 256, 1.0, stream, 0, n, buf.ptr, None))
    la.sync()
    return buf


def _check_structure(g, n):
    a0 = np.asarray(g["adj0"])
    valid = a0 != EMPTY
    assert (valid[:, :-1] >= valid[:, 1:]).all()  # compact lists
    assert (a0[valid] < n).all()
    assert not (a0 == np.arange(n, dtype=np.uint32)[:, None]).any()  # no self-edges
    srt = np.sort(np.where(valid, a0, EMPTY).astype(np.int64), axis=1)
    assert not ((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] != EMPTY)).any()  # no duplicate ids
    lv, uo, aU = np.asarray(g["levels"]), np.asarray(g["upper_off"]), np.asarray(g["adjU"])
    for v in np.nonzero(lv)[0]:
        for l in range(1, int(lv[v]) + 1):
            lst = aU[int(uo[v]) + l - 1]
            lst = lst[lst != EMPTY]
            assert (lst < n).all() and (lv[lst.astype(np.int64)] >= l).all() and (lst != v).all()
            assert len(set(lst.tolist())) == len(lst)


@pytest.mark.parametrize("kind,deg", [("hnsw", 48), ("hnsw", 64), ("vamana", 96), ("vamana", 128)])
def test_gpu_builder_wide_graph(la, po, gpu, kind, deg):
    n, d, efc = 20_000, 128, 128
    dX = _rows(la, n, d, 0)
    X, Q = dX.to_host(), _rows(la, 300, d, 1).to_host()
    truth = po.exact_topk(X, Q, 10)
    hnsw = kind == "hnsw"
    bt = la.BackendType.Hnsw if hnsw else la.BackendType.DiskAnn
    s = la.BackendSearcher.build_device(bt, dX.ptr, n, d, d, deg, efc)
    g = s.graph_export()
    M0 = 2 * deg if hnsw else deg
    assert g["M"] == deg and g["M0"] == M0
    _check_structure(g, n)
    assert _wide_lists(g["adj0"]) > 0
    mine = po.Graph.from_arrays(X, deg, M0, g["max_level"], g["entry"], g["levels"], g["upper_off"], g["adj0"], g["adjU"])
    # the GPU search over the built graph is the oracle walk of its export
    _assert_same(mine, s, Q, 10, 64, 0 if hnsw else 1)
    _assert_same(mine, s, np.concatenate([Q] * 4), 10, 128, 0 if hnsw else 1)
    seq = po.Graph.build_hnsw(X, M=deg, efc=efc) if hnsw else po.Graph.build_vamana(X, R=deg, L=efc, alpha=1.2)
    for ef in (32, 64):
        r_seq = recall_at_k(seq.search_batch(Q, 10, ef, 0, nthreads=8)[0], truth)
        r_gpu = recall_at_k(mine.search_batch(Q, 10, ef, 0, nthreads=8)[0], truth)
        print(f"{kind} {deg}: ef={ef} recall@10 sequential {r_seq:.4f} / GPU {r_gpu:.4f}")
        assert r_gpu >= r_seq - 0.01
    s.close()


def test_recall_at_degree_64_is_at_least_degree_32(la, po, gpu):
    """hard rows (65 536 clusters) and narrow beams, where a 20k-row set of easy rows saturates at recall 0.998 for both degrees"""
    n, d = 100_000, 128
    dX, dQ = la.DeviceArray((n, d), np.float32), la.DeviceArray((1000, d), np.float32)
    la._native.check(la.lib().leann_synth_rows_device(SEED, d, d, 64, 65536, 1.0, 0, 0, n, dX.ptr, None))
    la._native.check(la.lib().leann_synth_rows_device(SEED, d, d, 64, 65536, 1.0, 1, 0, 1000, dQ.ptr, None))
    la.sync()
    X, Q = dX.to_host(), dQ.to_host()
    truth = po.exact_topk(X, Q, 10)
    rec = {}
    for M in (32, 64):
        s = la.BackendSearcher.build_device(la.BackendType.Hnsw, dX.ptr, n, d, d, M, 128)
        rec[M] = [recall_at_k(s.search_batch(Q, 10, ef)[0], truth) for ef in (10, 16, 32)]
        s.close()
    print("recall@10 at ef 10/16/32:", rec)
    assert all(r64 >= r32 for r32, r64 in zip(rec[32], rec[64]))


def test_add_save_reopen_wide(la, po, gpu, tmp_path):
    """add_to_index in two parts at graph_degree 64: valid lists, the one-shot build's recall (test_gpu_robust.py's bar); save and
    reopen answers identically"""
    d, n0, n1, M = 64, 6000, 4000, 64
    X = synth(po, n0 + n1, d)
    Q = synth(po, 200, d, stream=1)
    B = la.BackendBuilder(la.BackendType.Hnsw)
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(); b.mkdir()
    B.build(X[:n0], [], str(a / "documents.leann"), d, M, 64)
    B.add_to_index(X[n0:], str(a / "documents.leann"), d, n0)
    B.build(X, [], str(b / "documents.leann"), d, M, 64)
    sa, sb = la.HnswSearcher.load(str(a / "documents.leann"), d), la.HnswSearcher.load(str(b / "documents.leann"), d)
    ga = sa.graph_export()
    assert sa.len() == n0 + n1 and ga["M0"] == 128
    _check_structure(ga, n0 + n1)
    truth = po.exact_topk(X, Q, 10)
    ka, _, _ = sa.search_batch(Q, 10, 64)
    kb, db, cb = sb.search_batch(Q, 10, 64)
    assert abs(recall_at_k(ka, truth) - recall_at_k(kb, truth)) <= 0.02 and recall_at_k(ka, truth) >= 0.95
    # an in-memory wide graph, saved and reopened: identical answers
    dX = la.DeviceArray.from_host(X)
    sm = la.BackendSearcher.build_device(la.BackendType.Hnsw, dX.ptr, n0 + n1, d, d, M, 64)
    km, dm, cm = sm.search_batch(Q, 10, 64)
    (tmp_path / "c").mkdir()
    sm.save(str(tmp_path / "c" / "documents.leann"))
    sb2 = la.HnswSearcher.load(str(tmp_path / "c" / "documents.leann"), d)
    k2, d2, c2 = sb2.search_batch(Q, 10, 64)
    assert (k2 == km).all() and (d2.view(np.uint32) == dm.view(np.uint32)).all() and (c2 == cm).all()
    sm.close()
    sa.close(); sb.close(); sb2.close()


def test_two_shard_composite_wide(la, po, gpu):
    n, d, nq, k, ef, M = 8192, 128, 64, 10, 96, 64
    X = synth(po, n, d)
    Q = synth(po, nq, d, stream=1)
    lows = [0, 4096, n]
    parts = [la.DeviceArray.from_host(X[lows[g]:lows[g + 1]]) for g in range(2)]
    sh = la.ShardedIndex.build_device(la.BackendType.Hnsw, [p.ptr for p in parts], [lows[g + 1] - lows[g] for g in range(2)], d, d, M, 64,
                                      [0, 0], keep=parts)
    s = sh.as_backend()
    gk, gd, gc = s.search_batch(Q, k, ef)
    ok, od, oc = [], [], []
    for g in range(2):
        gr = s.shard(g).graph_export()
        assert gr["M0"] == 128
        Gr = po.Graph.from_arrays(X[lows[g]:lows[g + 1]], M, 2 * M, gr["max_level"], gr["entry"], gr["levels"], gr["upper_off"],
                                  gr["adj0"], gr["adjU"])
        k0, d0, c0, _ = Gr.search_batch(Q, k, ef, 0, 4)
        ok.append(np.where(d0 == np.inf, np.iinfo(np.uint64).max, k0 + np.uint64(lows[g]))); od.append(d0); oc.append(c0)
    for q in range(nq):
        rk, rd = po.merge_topk(np.stack(ok)[:, q], np.stack(od)[:, q], np.stack(oc)[:, q], k)
        assert gc[q] == len(rk) and (gk[q, : len(rk)] == rk).all() and (gd[q, : len(rk)].view(np.uint32) == rd.view(np.uint32)).all()
    s.close()
    sh.close()


def test_cli_build_graph_degree_64(la, po, gpu, tmp_path):
    exe = os.path.join(ROOT, "leann-rs_amd", "host", "leann")
    topics = ["graph traversal beam hnsw neighbours", "gpu kernel wavefront lds bandwidth", "bm25 ranking term frequency"]
    docs = [dict(id=str(i + 1), text=f"passage {i} about {topics[i % 3]} number {i * 7919 % 1000}") for i in range(3000)]
    (tmp_path / "docs.jsonl").write_text("\n".join(json.dumps(x) for x in docs))
    r = subprocess.run([exe, "build", "--index-dir", str(tmp_path / "idx"), "--passages-jsonl", str(tmp_path / "docs.jsonl"),
                        "--dimensions", "96", "--graph-degree", "64", "--complexity", "64"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "search", "gpu kernel wavefront lds", "-i", str(tmp_path / "idx"), "--top-k", "5", "--format", "json"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    res = json.loads(r.stdout)
    assert len(res) == 5 and all("wavefront" in x["text"] for x in res)
    # the saved index is a wide graph, and searching it is the oracle walk of that graph
    s = la.HnswSearcher.load(str(tmp_path / "idx" / "documents.leann"), 96)
    g = s.graph_export(with_vectors=True)
    assert g["M"] == 64 and g["M0"] == 128
    _check_structure(g, 3000)
    G = po.Graph.from_arrays(g["vectors"], 64, 128, g["max_level"], g["entry"], g["levels"], g["upper_off"], g["adj0"], g["adjU"])
    _assert_same(G, s, g["vectors"][:200] + 0.01, 5, 64)
    s.close()


# ---- narrow builds are untouched --------------------------------------------------------------------------------------------------
def _graph_sha256(g):
    h = hashlib.sha256()
    h.update(np.array([g["n"], g["M"], g["M0"], g["max_level"], g["entry"]], np.uint64).tobytes())
    for k in ("levels", "upper_off", "adj0", "adjU"):
        h.update(np.ascontiguousarray(g[k]).tobytes())
    return h.hexdigest()


def test_narrow_builds_are_byte_identical_to_the_recorded_graphs(la, po, gpu):
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "narrow_build_sha256.json")))
    X = synth(po, 20000, 128)
    dX = la.DeviceArray.from_host(X)
    for name, bt, deg in (("hnsw_m16_n20000_d128", la.BackendType.Hnsw, 16), ("vamana_r32_n20000_d128", la.BackendType.DiskAnn, 32)):
        s = la.BackendSearcher.build_device(bt, dX.ptr, 20000, 128, 128, deg, 64)
        assert _graph_sha256(s.graph_export()) == want[name], name
        s.close()
