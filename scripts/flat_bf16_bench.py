#!/usr/bin/env python3
"""The flat search on bf16 rows (csrc/scan_bf16.hip) against the f32 exact scan and the flat search on int8 rows;
results go to profiles/flat_bf16.md.  Needs a GPU; fails without.  No thresholds: this prints what it measures.

    scripts/flat_bf16_bench.py --rows 1000000 10000000 --nq 64 256

Per shape: synthetic rows n x 768 in HBM (the f32 twin), an f32 HNSW handle H built on them — no leg reads its graph, so it is the
cheapest that builds (M = 4, efc = 8) —, to_rows(H, BF16) and to_rows(H, I8); nq queries, k = 10, fetch_k = 40.  Legs:
  flat bf16        leann_backend_search_flat_bf16_batch_device, no bitmap
  f32 scan         leann_scan_topk_device over the f32 twin, the same queries
  flat int8        leann_backend_search_flat_batch_device on the int8 twin
  flat bf16 1 % / 3 %   the new call under a shared bitmap allowing that share of the rows
Every call synchronises inside; a run is bracketed by device events on the null stream.  The legs alternate run by run: 3 warm-up runs
each, then --reps timed runs each; reported: median and spread (max - min).  Row bytes of a flat bf16 call: n x pitch x ceil(nq / 64),
against 8 TB/s.  Hardware counters are not read here: which of HBM, LDS and the matrix pipe binds the kernel stays unmeasured."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, D, K, FETCH, PEAK, BQ = 3, 768, 10, 40, 8e12, 64


def measure(hip, calls, reps):
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0
    times = {name: [] for name in calls}
    for r in range(WARMUP + reps):
        for name, fn in calls.items():
            assert hip.hipEventRecord(ev[0], None) == 0
            fn()
            assert hip.hipEventRecord(ev[1], None) == 0 and hip.hipEventSynchronize(ev[1]) == 0
            ms = C.c_float(0)
            assert hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
            if r >= WARMUP:
                times[name].append(ms.value)
    for e in ev:
        hip.hipEventDestroy(e)
    return {name: (statistics.median(t), max(t) - min(t)) for name, t in times.items()}


def recall(found, truth):
    return float(np.mean([len(set(f.tolist()) & set(t.tolist())) / K for f, t in zip(found, truth)]))


def run_shape(la, hip, n, nq, reps, out):
    L, chk = la.lib(), la._native.check
    X, Q = la.DeviceArray((n, D), np.float32), la.DeviceArray((nq, D), np.float32)
    chk(L.leann_synth_rows_device(0x5EED0001, D, D, 64, 4096, 1.0, 0, 0, n, X.ptr, None))
    chk(L.leann_synth_rows_device(0x5EED0001, D, D, 64, 4096, 1.0, 1, 0, nq, Q.ptr, None))
    la.sync()
    H = la.BackendSearcher.build_device(la.BackendType.Hnsw, X.ptr, n, D, D, 4, 8)
    b16, i8 = H.to_rows(la.RowType.BF16), H.to_rows(la.RowType.I8)
    keys, dists, counts = la.DeviceArray((nq, K), np.uint64), la.DeviceArray((nq, K), np.float32), la.DeviceArray(nq, np.uint32)
    flat16 = lambda allow=None: b16.search_flat_bf16_batch_device(Q.ptr, nq, K, FETCH, keys.ptr, dists.ptr, counts.ptr, d_allow=allow)
    flat8 = lambda: i8.search_flat_batch_device(Q.ptr, nq, K, FETCH, keys.ptr, dists.ptr, counts.ptr)
    scan = lambda allow=None: chk(L.leann_scan_topk_device(X.ptr, n, D, D, Q.ptr, nq, K, allow, 0, keys.ptr, dists.ptr, counts.ptr, None))
    answer = lambda fn, *a: (fn(*a), keys.to_host())[1]
    truth = answer(scan)
    legs = {"flat bf16": flat16, "f32 scan": scan, "flat int8": flat8}
    notes = [f"recall@10 against the f32 scan: flat bf16 {recall(answer(flat16), truth):.4f}, flat int8 {recall(answer(flat8), truth):.4f}"]
    held = []
    for pct in (1, 3):
        dbm = la.DeviceArray.from_host(np.packbits(np.random.default_rng(pct).random(n) < pct / 100, bitorder="little"))
        held.append(dbm)
        notes.append(f"{pct} % allowed: filtered recall@10 of flat bf16 against the f32 scan under the same bitmap "
                     f"{recall(answer(flat16, dbm.ptr), answer(scan, dbm.ptr)):.4f}")
        legs[f"flat bf16 {pct} %"] = lambda p=dbm.ptr: flat16(p)
    res = measure(hip, legs, reps)
    out.append(f"\n## {n} x {D}, nq = {nq}, k = {K}, fetch_k = {FETCH} ({reps} alternating runs)\n")
    out.append("| leg | median ms | spread ms | queries/s |\n|---|---|---|---|")
    for name, (med, spread) in res.items():
        out.append(f"| {name} | {med:.3f} | {spread:.3f} | {nq / med * 1e3:,.0f} |")
    row_bytes = n * ((D + 63) // 64 * 128) * ((nq + BQ - 1) // BQ)
    out.append(f"\nflat bf16: {row_bytes / 1e9:.2f} GB of row bytes per call = {row_bytes / (res['flat bf16'][0] * 1e-3) / PEAK:.3f} of 8 TB/s over "
               "the WHOLE call (split, screen, select, rescore and their synchronisations; not the kernel's share); f32 scan / flat bf16 = "
               f"{res['f32 scan'][0] / res['flat bf16'][0]:.2f} x; flat bf16 / flat int8 = {res['flat bf16'][0] / res['flat int8'][0]:.2f} x")
    out.extend("- " + x for x in notes)
    for s in (b16, i8, H):
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1000000, 10000000])
    ap.add_argument("--nq", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flat_bf16.md"))
    a = ap.parse_args()
    import leann_rs_amd as la
    if la.device_count() < 1:
        sys.exit("flat_bf16_bench: no HIP device visible")
    hip = la.lib()
    out = ["# Flat search on bf16 rows (scripts/flat_bf16_bench.py; protocol in its docstring)"]
    for n in a.rows:
        for nq in a.nq:
            run_shape(la, hip, n, nq, a.reps, out)
            with open(a.out, "w") as f:  # after every shape: a later one that fails leaves the earlier ones
                f.write("\n".join(out) + "\n\nNot measured: kernel times on their own (rocprofv3) — score_bf16_mfma_kernel's among them —, "
                        "hardware counters (which of HBM, LDS and the matrix pipe binds it), other widths than 768, fetch_k other than 40.\n")


if __name__ == "__main__":
    main()
