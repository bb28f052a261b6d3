#!/usr/bin/env python3
"""Exact search under per-query filters: this tree's library against a library built from the parent commit (results in
profiles/exact_lists.md; the protocol is profiles/meta_batch.md's).  Needs a GPU; fails without.

    make -C <checkout of the parent commit> leann-rs_amd/csrc/libleann_hip.so
    scripts/exact_lists_bench.py --parent-lib <that checkout>/leann-rs_amd/csrc/libleann_hip.so --rows 1000000 10000000

Both libraries are loaded into one process and given the same device rows (synthetic, R x 768), each its own HNSW handle (M = 16,
efc = 64) and metadata store (tenant: 1000 distinct strings; year).  64 queries, k = 10:
  a  64 distinct filters tenant == t_i AND year >= c_i, one leann_backend_search_meta_batch_device call, mode 1
  b  the same 64 queries over 8 distinct filters (query i under filter i % 8), the same call
  b-lists (this tree only)  shape b as one leann_backend_search_exact_lists_batch_device call: 8 lists, q_list = i % 8
A run is bracketed by device events on the null stream (the calls synchronise inside).  The sides alternate run by run: 5 warm-up
runs each, then --reps timed runs each; reported: median and spread (max - min).  Before timing, the two sides' keys, distance bits
and counts are compared.  Algorithmic bytes: the allowed rows of every query, 768 x 4 bytes each, against 8 TB/s."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.meta_batch_bench import filters_for, make_store, stats  # noqa: E402

WARMUP, D, NQ, K, PEAK = 5, 768, 64, 10, 8e12


class Side:
    """one library: la's wrappers call it while `with side:` is open"""

    def __init__(self, la, path):
        self.N = la._native
        self.L = self.N.lib() if path is None else C.CDLL(path)
        for name, (res, args) in self.N.SIGNATURES.items() if path else ():
            if hasattr(self.L, name):
                f = getattr(self.L, name)
                f.restype, f.argtypes = res, args

    def __enter__(self):
        self.prev, self.N._lib = self.N._lib, self.L

    def __exit__(self, *exc):
        self.N._lib = self.prev


def measure(la, hip, sides, calls, reps):
    """calls: {side name: callable}; -> {name: stats} over device-event times, the sides alternating"""
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0
    times = {name: [] for name in calls}
    for r in range(WARMUP + reps):
        for name, fn in calls.items():
            with sides[name.split()[0]]:
                assert hip.hipEventRecord(ev[0], None) == 0
                fn()
                assert hip.hipEventRecord(ev[1], None) == 0 and hip.hipEventSynchronize(ev[1]) == 0
            ms = C.c_float(0)
            assert hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
            if r >= WARMUP:
                times[name].append(ms.value * 1e-3)
    for e in ev:
        hip.hipEventDestroy(e)
    return {name: stats(t) for name, t in times.items()}


def run_rows(la, hip, sides, n, reps):
    X, Q = la.DeviceArray((n, D), np.float32), la.DeviceArray((NQ, D), np.float32)
    L = la.lib()
    la._native.check(L.leann_synth_rows_device(0x5EED0001, D, D, 64, 4096, 1.0, 0, 0, n, X.ptr, None))
    la._native.check(L.leann_synth_rows_device(0x5EED0001, D, D, 64, 4096, 1.0, 1, 0, NQ, Q.ptr, None))
    la.sync()
    own = {}
    for name, side in sides.items():
        with side:
            m, tenant, year = make_store(la, n)
            own[name] = (la.BackendSearcher.build_device(la.BackendType.Hnsw, X.ptr, n, D, D, 16, 64), m)
    out = dict(rows=n)
    for shape, distinct in (("a", NQ), ("b", 8)):
        flt = [filters_for(distinct)[i % distinct] for i in range(NQ)]
        nodes, off, _, keep = la.metadata.encode_trees(flt)
        res = {name: (la.DeviceArray((NQ, K), np.uint64), la.DeviceArray((NQ, K), np.float32), la.DeviceArray(NQ, np.uint32)) for name in sides}
        allowed = la.DeviceArray(NQ, np.uint32)

        def call(name):
            s, m = own[name]
            k, d, c = res[name]
            return lambda: la._native.check(sides[name].L.leann_backend_search_meta_batch_device(s._h, m._h, Q.ptr, NQ, K, 64, nodes, off, 1, k.ptr,
                                                                                                 d.ptr, c.ptr, None, allowed.ptr, None))
        calls = {name: call(name) for name in sides}
        if shape == "b":  # the lists call over the 8 distinct filters' positions, q_list = i % 8
            s, m = own["candidate"]
            bms = m.eval_batch(flt[:8])
            lists = [np.flatnonzero(np.unpackbits(b, bitorder="little")[:n]).astype(np.uint32) for b in bms]
            loff = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64)
            d_lists, ql = la.DeviceArray.from_host(np.concatenate(lists)), (np.arange(NQ) % 8).astype(np.uint32)
            lk, ld_, lc = la.DeviceArray((NQ, K), np.uint64), la.DeviceArray((NQ, K), np.float32), la.DeviceArray(NQ, np.uint32)
            calls["candidate lists"] = lambda: s.search_exact_lists_batch_device(Q.ptr, NQ, K, loff, d_lists.ptr, 8, ql, lk.ptr, ld_.ptr, lc.ptr)
            res["candidate lists"] = (lk, ld_, lc)
        for name, fn in calls.items():
            with sides[name.split()[0]]:
                fn()
        la.sync()
        first = [a.to_host() for a in res["parent"]]
        for name in res:
            got = [a.to_host() for a in res[name]]
            assert all((g.view(np.uint32) == f.view(np.uint32)).all() for g, f in zip(got, first)), f"{name}: answers differ from the parent's"
        t = measure(la, hip, sides, calls, reps)
        rows_read = int(allowed.to_host().astype(np.int64).sum())
        for name, st in t.items():
            st["share_of_8TBps"] = rows_read * D * 4 / (st["median_ms"] * 1e-3) / PEAK
        p, c = t["parent"], t["candidate"]
        out[shape] = dict(distinct_filters=distinct, allowed_rows_total=rows_read, algorithmic_bytes=rows_read * D * 4, **t,
                          faster_by_more_than_both_spreads=bool(p["median_ms"] - c["median_ms"] > p["spread_ms"] + c["spread_ms"]))
        print(json.dumps({shape: out[shape]}), flush=True)
        del keep
    for name, (s, m) in own.items():
        with sides[name]:
            s.close()
            m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libleann_hip.so built from the parent commit")
    ap.add_argument("--rows", type=int, nargs="*", default=[1_000_000, 10_000_000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import leann_rs_amd as la
    if la.device_count() < 1:
        raise SystemExit("exact_lists_bench: no HIP device visible")
    hip = C.CDLL("libamdhip64.so")
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventDestroy.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    sides = dict(parent=Side(la, a.parent_lib), candidate=Side(la, None))
    out = dict(reps=a.reps, warmup=WARMUP, results=[run_rows(la, hip, sides, n, a.reps) for n in a.rows])
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
