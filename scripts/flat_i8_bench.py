#!/usr/bin/env python3
"""The flat search on int8 rows (csrc/scan_i8.hip) against the f32 exact scan and the filtered int8 walk; results go to
profiles/flat_i8.md.  Needs a GPU; fails without.  No thresholds: this prints what it measures.

    scripts/flat_i8_bench.py --rows 1000000 10000000 --nq 64 256

Per shape: synthetic rows n x 768 in HBM (the f32 twin), an int8 HNSW handle built from them (M = 16, efc = 64), nq queries, k = 10,
fetch_k = 40.  Legs:
  flat        leann_backend_search_flat_batch_device, no bitmap
  f32 scan    leann_scan_topk_device over the f32 twin, the same queries
  flat 1 % / 3 %   the flat call under a shared bitmap allowing that share of the rows
  walk 1 % / 3 %   leann_backend_search_filtered_batch_device on the same handle at the smallest ef of 64, 128, 256, 512, 1024 whose
                   filtered recall@10 (against the f32 scan under the same bitmap) reaches the flat call's; "none" if no ef does
Every call synchronises inside; a run is bracketed by device events on the null stream.  The legs alternate run by run: 3 warm-up runs
each, then --reps timed runs each; reported: median and spread (max - min).  Row bytes of a flat call: n x ldb x ceil(nq / 64), against
8 TB/s.  Hardware counters are not read here: which of HBM, LDS and the matrix pipe binds the kernel stays unmeasured."""
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
    s = la.BackendSearcher.build_device(la.BackendType.Hnsw, X.ptr, n, D, D, 16, 64, row_type=la.RowType.I8)
    keys, dists, counts = la.DeviceArray((nq, K), np.uint64), la.DeviceArray((nq, K), np.float32), la.DeviceArray(nq, np.uint32)
    flat = lambda allow=None: s.search_flat_batch_device(Q.ptr, nq, K, FETCH, keys.ptr, dists.ptr, counts.ptr, d_allow=allow)
    scan = lambda allow=None: chk(L.leann_scan_topk_device(X.ptr, n, D, D, Q.ptr, nq, K, allow, 0, keys.ptr, dists.ptr, counts.ptr, None))
    walk = lambda ef, allow: (s.search_filtered_batch_device(Q.ptr, nq, K, ef, allow, 0, keys.ptr, dists.ptr, counts.ptr), la.sync())
    answer = lambda fn, *a: (fn(*a), keys.to_host())[1]
    truth = answer(scan)
    legs = {"flat": flat, "f32 scan": scan}
    notes = [f"recall@10 of flat against the f32 scan: {recall(answer(flat), truth):.4f}"]
    held = []
    for pct in (1, 3):
        bm = np.packbits(np.random.default_rng(pct).random(n) < pct / 100, bitorder="little")
        dbm = la.DeviceArray.from_host(bm)
        held.append(dbm)
        t = answer(scan, dbm.ptr)
        r_flat = recall(answer(flat, dbm.ptr), t)
        legs[f"flat {pct} %"] = lambda p=dbm.ptr: flat(p)
        pick = None
        for ef in (64, 128, 256, 512, 1024):
            r_walk = recall(answer(walk, ef, dbm.ptr), t)
            notes.append(f"{pct} % allowed: walk ef = {ef} filtered recall {r_walk:.4f} (flat {r_flat:.4f})")
            if r_walk >= r_flat:
                pick = ef
                break
        if pick:
            legs[f"walk {pct} % (ef = {pick})"] = lambda p=dbm.ptr, ef=pick: walk(ef, p)
        else:
            notes.append(f"{pct} % allowed: no ef up to 1024 reaches the flat call's recall; the walk is not timed")
    res = measure(hip, legs, reps)
    ldb = (D + 127) // 128 * 128
    out.append(f"\n## {n} x {D}, nq = {nq}, k = {K}, fetch_k = {FETCH} ({reps} alternating runs)\n")
    out.append("| leg | median ms | spread ms | queries/s |\n|---|---|---|---|")
    for name, (med, spread) in res.items():
        out.append(f"| {name} | {med:.3f} | {spread:.3f} | {nq / med * 1e3:,.0f} |")
    row_bytes = n * ldb * ((nq + BQ - 1) // BQ)
    out.append(f"\nflat: {row_bytes / 1e9:.2f} GB of row bytes per call = {row_bytes / (res['flat'][0] * 1e-3) / PEAK:.3f} of 8 TB/s over the WHOLE "
               "call (quantise, screen, select, rescore and their synchronisations; not the kernel's share); flat / f32 scan = "
               f"{res['f32 scan'][0] / res['flat'][0]:.2f} x")
    out.extend("- " + x for x in notes)
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1000000, 10000000])
    ap.add_argument("--nq", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flat_i8.md"))
    a = ap.parse_args()
    import leann_rs_amd as la
    if la.device_count() < 1:
        sys.exit("flat_i8_bench: no HIP device visible")
    hip = la.lib()
    out = ["# Flat search on int8 rows (scripts/flat_i8_bench.py; protocol in its docstring)"]
    for n in a.rows:
        for nq in a.nq:
            run_shape(la, hip, n, nq, a.reps, out)
            with open(a.out, "w") as f:  # after every shape: a later one that fails leaves the earlier ones
                f.write("\n".join(out) + "\n\nNot measured: kernel times on their own (rocprofv3), hardware counters (which of HBM, LDS and "
                        "the matrix pipe binds score_i8_mfma_kernel), other widths than 768, fetch_k other than 40.\n")


if __name__ == "__main__":
    main()
