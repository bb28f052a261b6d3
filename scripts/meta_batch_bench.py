#!/usr/bin/env python3
"""A batch of per-query metadata filters: one leann_meta_eval_batch_device call against one leann_meta_eval_device call per filter
(DESIGN.md §3c "A batch of filters"; results in profiles/meta_batch.md).  Needs a GPU; fails without.

Store: --rows passages with a string column `tenant` (1000 distinct values) and a numeric column `year`.  Filters: tenant == t_i AND
year >= c_i, F distinct ones for F in 1, 8, 64.  The trees are encoded once, outside the timed window; both sides call the C ABI
through ctypes on the null stream of one process, and a timed run is the host clock from before the first call to the end of a
device synchronise.
  baseline   F calls of leann_meta_eval_device back to back, each into its own row of the output block (what a caller does today)
  candidate  one leann_meta_eval_batch_device call into the same block
The two alternate, run by run: 5 warm-up runs each, then --reps timed runs each.  Reported per side: the median and the spread (max -
min over the timed runs).  The condition for F = 64: median(baseline) - median(candidate) > spread(baseline) + spread(candidate).
Before timing, the candidate's bitmaps and counts are compared with the baseline's, bit for bit.

--e2e-rows R (0 = skip): on an R x 768 HNSW index (synthetic rows, M = 16, efc = 64), 64 queries under 64 filters: one
leann_backend_search_meta_batch_device call against 64 x (leann_meta_eval_device + a one-query
leann_backend_search_filtered_batch_device); reported, no condition."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TENANTS = 1000
WARMUP = 5


def make_store(la, n):
    rng = np.random.default_rng(3)
    tenant = rng.integers(0, TENANTS, n)
    year = rng.integers(2000, 2025, n).astype(np.float64)
    names = np.array([f"t{i:04d}".encode() for i in range(TENANTS)], dtype="S5")
    m = la.MetaColumns(n)
    m.add_column("tenant", np.full(n, 5, np.uint8), None, names[tenant].tobytes(), np.arange(n + 1, dtype=np.uint64) * np.uint64(5))
    m.add_column("year", np.full(n, 4, np.uint8), year)
    return m, tenant, year


def filters_for(k):
    return [("and", [("cond", "tenant", "eq", f"t{(37 * i) % TENANTS:04d}"), ("cond", "year", "gte", 2000 + (5 * i) % 25)]) for i in range(k)]


def stats(times):
    t = np.array(times) * 1e3
    return dict(median_ms=float(np.median(t)), spread_ms=float(t.max() - t.min()), min_ms=float(t.min()), max_ms=float(t.max()))


def eval_part(la, n, reps, out):
    L = la.lib()
    m, tenant, year = make_store(la, n)
    nbytes = (n + 7) // 8
    stride = (nbytes + 15) // 16 * 16
    rows = []
    for k in (1, 8, 64):
        flt = filters_for(k)
        single = [la.metadata.encode_tree(f) for f in flt]
        nodes, off, _, keep = la.metadata.encode_trees(flt)
        d_a, d_b = la.DeviceArray(k * stride, np.uint8), la.DeviceArray(k * stride, np.uint8)
        c_a, c_b = la.DeviceArray(k, np.uint32), la.DeviceArray(k, np.uint32)
        distinct = C.c_size_t(0)

        def baseline():
            for i, (nd, cnt, _) in enumerate(single):
                la._native.check(L.leann_meta_eval_device(m._h, nd, cnt, None, d_a.ptr + i * stride, c_a.ptr + 4 * i, None))
            la.sync()

        def candidate():
            la._native.check(L.leann_meta_eval_batch_device(m._h, nodes, off, k, None, d_b.ptr, stride, c_b.ptr, C.byref(distinct), None))
            la.sync()
        baseline()
        candidate()
        a, b = d_a.to_host().reshape(k, stride)[:, :nbytes], d_b.to_host().reshape(k, stride)[:, :nbytes]
        assert (a == b).all() and (c_a.to_host() == c_b.to_host()).all(), "the batch's answers differ from the single calls'"
        want0 = int(((tenant == 0) & (year >= 2000)).sum())  # filter 0: tenant == t0000 AND year >= 2000
        assert int(c_b.to_host()[0]) == want0, (int(c_b.to_host()[0]), want0)
        tb, tc = [], []
        for r in range(WARMUP + reps):
            t = time.perf_counter()
            baseline()
            t1 = time.perf_counter()
            candidate()
            t2 = time.perf_counter()
            if r >= WARMUP:
                tb.append(t1 - t)
                tc.append(t2 - t1)
        sb, sc = stats(tb), stats(tc)
        row = dict(rows=n, filters=k, distinct=int(distinct.value), baseline=sb, candidate=sc, ratio=sb["median_ms"] / sc["median_ms"],
                   faster_by_more_than_both_spreads=bool(sb["median_ms"] - sc["median_ms"] > sb["spread_ms"] + sc["spread_ms"]))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del keep
    m.close()
    out.setdefault("eval", []).extend(rows)


def e2e_part(la, n, reps, out):
    L = la.lib()
    d, nq, k, ef = 768, 64, 10, 64
    m, _, _ = make_store(la, n)
    X = la.DeviceArray((n, d), np.float32)
    Q = la.DeviceArray((nq, d), np.float32)
    la._native.check(L.leann_synth_rows_device(0x5EED0001, d, d, 64, 4096, 1.0, 0, 0, n, X.ptr, None))
    la._native.check(L.leann_synth_rows_device(0x5EED0001, d, d, 64, 4096, 1.0, 1, 0, nq, Q.ptr, None))
    la.sync()
    t = time.perf_counter()
    s = la.BackendSearcher.build_device(la.BackendType.Hnsw, X.ptr, n, d, d, 16, 64)
    build_s = time.perf_counter() - t
    flt = filters_for(nq)
    single = [la.metadata.encode_tree(f) for f in flt]
    nodes, off, _, keep = la.metadata.encode_trees(flt)
    nbytes = (n + 7) // 8
    d_bm = la.DeviceArray(nbytes, np.uint8)
    ka, da, ca = la.DeviceArray((nq, k), np.uint64), la.DeviceArray((nq, k), np.float32), la.DeviceArray(nq, np.uint32)
    kb, db, cb = la.DeviceArray((nq, k), np.uint64), la.DeviceArray((nq, k), np.float32), la.DeviceArray(nq, np.uint32)
    res = {}
    for mode, name in ((0, "walk"), (1, "exact")):
        def baseline():
            for i, (nd, cnt, _) in enumerate(single):
                la._native.check(L.leann_meta_eval_device(m._h, nd, cnt, None, d_bm.ptr, None, None))
                if mode == 0:
                    la._native.check(L.leann_backend_search_filtered_batch_device(s._h, Q.ptr + i * d * 4, 1, k, ef, d_bm.ptr, 0, ka.ptr + i * k * 8,
                                                                                  da.ptr + i * k * 4, ca.ptr + i * 4, None, None))
                else:
                    la._native.check(L.leann_backend_search_filtered_exact_batch_device(s._h, Q.ptr + i * d * 4, 1, k, d_bm.ptr, 0,
                                                                                        ka.ptr + i * k * 8, da.ptr + i * k * 4, ca.ptr + i * 4, None))
            la.sync()

        def candidate():
            la._native.check(L.leann_backend_search_meta_batch_device(s._h, m._h, Q.ptr, nq, k, ef, nodes, off, mode, kb.ptr, db.ptr, cb.ptr,
                                                                      None, None, None))
        baseline()
        candidate()
        same = bool((ka.to_host() == kb.to_host()).all() and (ca.to_host() == cb.to_host()).all())
        tb, tc = [], []
        for r in range(WARMUP + reps):
            t = time.perf_counter()
            baseline()
            t1 = time.perf_counter()
            candidate()
            t2 = time.perf_counter()
            if r >= WARMUP:
                tb.append(t1 - t)
                tc.append(t2 - t1)
        res[name] = dict(baseline=stats(tb), candidate=stats(tc), same_keys_and_counts_as_one_query_calls=same)
        print(json.dumps({name: res[name]}), flush=True)
    out["e2e"] = dict(rows=n, dims=d, queries=nq, top_k=k, ef=ef, build_s=build_s, **res)
    del keep
    s.close()
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[1_000_000, 10_000_000])  # (--rows alone: skip the evaluation part)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--e2e-rows", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import leann_rs_amd as la
    if la.device_count() < 1:
        raise SystemExit("meta_batch_bench: no HIP device visible")
    out = dict(reps=a.reps, warmup=WARMUP)
    for n in a.rows:
        eval_part(la, n, a.reps, out)
    if a.e2e_rows:
        e2e_part(la, a.e2e_rows, a.reps, out)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
