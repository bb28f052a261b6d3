"""Delete consolidation on one MI355X: HNSW M = 32 on N x 768 clustered synthetic rows, a random 1 % and 10 % removed.
Per fraction: seconds of leann_backend_consolidate against a rebuild of the live rows with the same builder; queries/s and recall@10
of the plain search after the repair against the filtered walk over the un-repaired tombstones at the same ef (16 384 queries per
call, recall on the first 1 000 against the exact scan of the live rows); and the repair's gather traffic — for every repaired
level-0 list, the live ids of its own list and of its removed neighbours' lists (every slot, an upper bound: ids already in the pool
are not gathered again), plus the NC rows of its Gram matrix, times the row bytes — per second of the whole consolidate call
(upper levels, snapshot copies and the mark / clear passes included), as a fraction of the 6.4 TB/s whole-row gather ceiling
(profiles/r02_gather_ceiling.txt).  Appends to profiles/r06_delete_consolidate.md.
Usage: python scripts/exp/delete_consolidate.py [--n 1000000] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import leann_rs_amd as la  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--d", type=int, default=768)
ap.add_argument("--M", type=int, default=32)
ap.add_argument("--ef", type=int, default=64)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_delete_consolidate.md"))
a = ap.parse_args()
L, chk = la.lib(), la._native.check
SEED, NQ, NR, K, EMPTY = 0x5EED0001, 16384, 1000, 10, 0xFFFFFFFF


def emit(s):
    print(s, flush=True)
    with open(a.out, "a") as f:
        f.write(s + "\n")


def rows(n, stream):
    buf = la.DeviceArray((n, a.d), np.float32)
    chk(L.leann_synth_rows_device(SEED, a.d, a.d, 64, 4096, 1.0, stream, 0, n, buf.ptr, None))
    la.sync()
    return buf


def timed_search(s, Q):
    ok, od, oc = la.DeviceArray((NQ, K), np.uint64), la.DeviceArray((NQ, K), np.float32), la.DeviceArray(NQ, np.uint32)
    s.search_batch_device(Q.ptr, NQ, K, a.ef, ok.ptr, od.ptr, oc.ptr)
    la.sync()
    t = time.perf_counter()
    for _ in range(5):
        s.search_batch_device(Q.ptr, NQ, K, a.ef, ok.ptr, od.ptr, oc.ptr)
    la.sync()
    return 5 * NQ / (time.perf_counter() - t), ok.to_host()


def recall(keys, truth):
    return float(np.mean([len(set(x.tolist()) & set(y.tolist())) / K for x, y in zip(keys[:NR], truth[:NR])]))


emit(f"\n## {a.n} x {a.d}, HNSW M = {a.M}, ef = {a.ef} (scripts/exp/delete_consolidate.py)\n")
dX, Q = rows(a.n, 0), rows(NQ, 1)
for frac in (0.01, 0.10):
    t = time.perf_counter()
    s = la.BackendSearcher.build_device(la.BackendType.Hnsw, dX.ptr, a.n, a.d, a.d, a.M, 64)
    t_build = time.perf_counter() - t
    removed = np.zeros(a.n, bool)
    removed[np.random.default_rng(1).choice(a.n, int(a.n * frac), replace=False)] = True
    s.remove(np.flatnonzero(removed).astype(np.uint64))
    ones = la.DeviceArray.from_host(np.full((a.n + 7) // 8, 0xFF, np.uint8))
    tk, td, tc = la.DeviceArray((NR, K), np.uint64), la.DeviceArray((NR, K), np.float32), la.DeviceArray(NR, np.uint32)
    s.search_filtered_exact_batch_device(Q.ptr, NR, K, ones.ptr, 0, tk.ptr, td.ptr, tc.ptr)  # exact over the live rows
    la.sync()
    truth = tk.to_host()
    qps_t, keys_t = timed_search(s, Q)
    g = s.graph_export()
    adj, M0 = g["adj0"], g["M0"]
    safe = np.where(adj == EMPTY, 0, adj)
    dead_e = (adj != EMPTY) & removed[safe]
    live_cnt = ((adj != EMPTY) & ~dead_e).sum(1)
    touched = ~removed & dead_e.any(1)
    gathered = (live_cnt + (np.where(dead_e, live_cnt[safe], 0)).sum(1))[touched].sum() + int(touched.sum()) * (256 if M0 > 64 else 128)
    t = time.perf_counter()
    s.consolidate()
    t_cons = time.perf_counter() - t
    assert s.removed_bitmap()[1] == 0
    qps_c, keys_c = timed_search(s, Q)
    s.close()
    live = np.flatnonzero(~removed)
    dL = la.DeviceArray.from_host(dX.to_host()[live])
    t = time.perf_counter()
    r = la.BackendSearcher.build_device(la.BackendType.Hnsw, dL.ptr, len(live), a.d, a.d, a.M, 64)
    t_re = time.perf_counter() - t
    qps_r, keys_r = timed_search(r, Q)
    r.close()
    keys_r = np.where(keys_r == np.iinfo(np.uint64).max, keys_r, live[np.minimum(keys_r, len(live) - 1).astype(np.int64)].astype(np.uint64))
    tb = gathered * a.d * 4 / t_cons / 1e12
    emit(f"* {frac:.0%} removed ({int(removed.sum())} rows; build of all rows {t_build:.2f} s): consolidate {t_cons:.3f} s against a rebuild of "
         f"the live rows {t_re:.2f} s; {int(touched.sum())} level-0 lists repaired, {gathered * a.d * 4 / 1e9:.1f} GB of row gathers "
         f"(upper bound) = {tb:.2f} TB/s = {tb / 6.4:.0%} of the 6.4 TB/s gather ceiling")
    emit(f"  * filtered walk over the tombstones: {qps_t / 1e3:.0f} k q/s, recall@10 {recall(keys_t, truth):.4f}; plain search after the "
         f"repair: {qps_c / 1e3:.0f} k q/s, recall@10 {recall(keys_c, truth):.4f}; rebuilt graph: {qps_r / 1e3:.0f} k q/s, "
         f"recall@10 {recall(keys_r, truth):.4f}")
