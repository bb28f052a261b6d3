"""Wide graphs (lists of more than 64 ids) against today's degrees, 1M rows on one GPU: build seconds, then recall@10 and queries/s
along an ef ladder (16 384 queries per call, recall on the first 2 000 against the exact scan).
  * HNSW 1M x 768 at M in {32, 48, 64}, clustered synthetic rows (r = 64, 4 096 clusters) and the hard 65 536-cluster variant;
  * recompute-on graph (no stored vectors, h = 256 bf16 features, d = 768) at graph_degree 32 against 64;
  * DiskANN 1M x 1536 at R in {64, 128}.
Writes profiles/r04_wide_degree.txt (and prints every line as it goes).  Usage: python scripts/exp/wide_degree.py [out]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import leann_rs_amd as la  # noqa: E402

L, chk = la.lib(), la._native.check
SEED, NQ, NR, K, N = 0x5EED0001, 16384, 2000, 10, 1_000_000
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r04_wide_degree.txt")
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write("# scripts/exp/wide_degree.py on one MI355X: build seconds; recall@10 (first 2 000 of 16 384 queries, exact truth) and q/s per ef\n")


def emit(s):
    print(s, flush=True)
    with open(OUT, "a") as f:  # line by line: a partial run leaves what it measured
        f.write(s + "\n")


def recall(keys, truth):
    return float(np.mean([len(set(a.tolist()) & set(b.tolist())) / K for a, b in zip(keys[:NR], truth[:NR])]))


def ladder(s, Q, truth, efs):
    ok, od, oc = la.DeviceArray((NQ, K), np.uint64), la.DeviceArray((NQ, K), np.float32), la.DeviceArray(NQ, np.uint32)
    out = []
    for ef in efs:
        s.search_batch_device(Q.ptr, NQ, K, ef, ok.ptr, od.ptr, oc.ptr)  # warm-up
        la.sync()
        t0 = time.perf_counter()
        for _ in range(5):
            s.search_batch_device(Q.ptr, NQ, K, ef, ok.ptr, od.ptr, oc.ptr)
        la.sync()
        qps = NQ * 5 / (time.perf_counter() - t0)
        out.append(f"ef={ef} recall={recall(ok.to_host(), truth):.4f} {qps / 1e6:.3f}M q/s")
    return "; ".join(out)


def exact(X, d, Q):
    tk, ts, tc = la.DeviceArray((NR, K), np.uint64), la.DeviceArray((NR, K), np.float32), la.DeviceArray(NR, np.uint32)
    chk(L.leann_scan_topk_device(X.ptr, N, d, d, Q.ptr, NR, K, None, 0, tk.ptr, ts.ptr, tc.ptr, None))
    la.sync()
    return tk.to_host()


def rows(d, clusters, stream, n):
    A = la.DeviceArray((n, d), np.float32)
    chk(L.leann_synth_rows_device(SEED, d, d, 64, clusters, 1.0, stream, 0, n, A.ptr, None))
    la.sync()
    return A


EFS = (16, 24, 32, 48, 64, 96, 128)
for clusters in (4096, 65536):
    d = 768
    X, Q = rows(d, clusters, 0, N), rows(d, clusters, 1, NQ)
    truth = exact(X, d, Q)
    for M in (32, 48, 64):
        t0 = time.time()
        s = la.BackendSearcher.build_device(la.BackendType.Hnsw, X.ptr, N, d, d, M, 128)
        tb = time.time() - t0
        emit(f"hnsw 1M x 768 clusters={clusters} M={M} efc=128: build {tb:.1f} s | {ladder(s, Q, truth, EFS)}")
        s.close()
    del X, Q

# recompute-on graph: queries are embeddings of query-side features; truth = the exact recompute search over the same encoder
h, d = 256, 768
F, W, Fq = la.DeviceArray((N, h), np.int16), la.DeviceArray((h, d), np.int16), la.DeviceArray((NQ, h), np.int16)
chk(L.leann_synth_features_device(SEED, h, 64, 4096, 1.0, 0, 0, N, F.ptr, None))
chk(L.leann_synth_weights_device(SEED, h, d, W.ptr, None))
chk(L.leann_synth_features_device(SEED, h, 64, 4096, 1.0, 1, 0, NQ, Fq.ptr, None))
la.sync()
r, rq = C.c_void_p(), C.c_void_p()
chk(L.leann_recompute_create(F.ptr, N, h, W.ptr, d, 0, 0, C.byref(r)))
chk(L.leann_recompute_create(Fq.ptr, NQ, h, W.ptr, d, 0, 0, C.byref(rq)))
Q = la.DeviceArray((NQ, d), np.float32)
chk(L.leann_recompute_encode_device(rq, 0, NQ, Q.ptr, None))
tk, ts, tc = la.DeviceArray((NR, K), np.uint64), la.DeviceArray((NR, K), np.float32), la.DeviceArray(NR, np.uint32)
chk(L.leann_recompute_search_batch_device(r, Q.ptr, NR, K, None, tk.ptr, ts.ptr, tc.ptr, None))
la.sync()
truth = tk.to_host()
for deg in (32, 64):
    hb = C.c_void_p()
    t0 = time.time()
    chk(L.leann_recompute_build_index(r, 0, deg, 128, C.byref(hb)))
    tb = time.time() - t0
    s = la.BackendSearcher(hb, la.BackendType.Hnsw)
    emit(f"recompute-on graph 1M h=256 d=768 M={deg} efc=128: build {tb:.1f} s | {ladder(s, Q, truth, EFS)}")
    s.close()
L.leann_recompute_close(r)
L.leann_recompute_close(rq)
del F, W, Fq, Q

d = 1536
X, Q = rows(d, 4096, 0, N), rows(d, 4096, 1, NQ)
truth = exact(X, d, Q)
for R in (64, 128):
    t0 = time.time()
    s = la.BackendSearcher.build_device(la.BackendType.DiskAnn, X.ptr, N, d, d, R, 128)
    tb = time.time() - t0
    emit(f"diskann 1M x 1536 R={R} L=128: build {tb:.1f} s | {ladder(s, Q, truth, (32, 48, 64, 96, 128))}")
    s.close()

