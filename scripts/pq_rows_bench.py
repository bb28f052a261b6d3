#!/usr/bin/env python3
"""PQ rows (csrc/scan_pq.hip) against sign-bit rows, MXFP4 rows and the int8 flat search on the same rows in the same
process; results go to profiles/pq_rows.md.  Needs a GPU; fails without.  No thresholds: this prints what it measures.

    scripts/pq_rows_bench.py --rows 1000000 10000000 --nq 64 256

Per shape: synthetic rows n x 768 in HBM from leann_synth_rows_device, codebooks for dsub = 8 and 4 trained on the first 65 536 rows
(leann_pq_train_device, iters = 8, timed once: "train"), their PQ codes (leann_pq_rows_from_device, timed: "encode"), their sign bits,
their MXFP4 codes, an int8 HNSW handle built from the same rows (M = 16, efc = 64; only up to --i8-max-rows rows), nq queries.  Legs,
fetch_k = 40, no bitmap: leann_pq_rows_search_batch_device at dsub 8 and 4, leann_bit_rows_search_batch_device,
leann_mx4_rows_search_batch_device, leann_backend_search_flat_batch_device (top_k = 10).
Every call synchronises inside; a run is bracketed by device events on the null stream.  The legs alternate run by run: 3 warm-up runs
each, then --reps timed runs each; reported: median and spread (max - min).  These are WHOLE calls (query tables, score, select and
their synchronisations), not kernel times.
Recall@10 against leann_scan_topk_device on the f32 rows at fetch_k = 40, 100, 400: every object's refined call on the exact rows in
HBM.  Synthetic clustered rows: no promise about a real embedding model."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bit_rows_bench import D, K, measure, recall  # noqa: E402

FETCH, RECALL_FETCHES, SAMPLE, ITERS = 40, (40, 100, 400), 65536, 8


def run_shape(la, hip, a, n, nq, out):
    L, chk = la.lib(), la._native.check
    X, Q = la.DeviceArray((n, D), np.float32), la.DeviceArray((nq, D), np.float32)
    chk(L.leann_synth_rows_device(0x5EED0001, D, D, 64, 4096, 1.0, 0, 0, n, X.ptr, None))
    chk(L.leann_synth_rows_device(0x5EED0001, D, D, 64, 4096, 1.0, 1, 0, nq, Q.ptr, None))
    la.sync()
    pq, notes = {}, []
    for dsub in (8, 4):
        cb = np.zeros((D // dsub, 256, dsub), np.float32)
        train = measure(hip, {"train": lambda: chk(L.leann_pq_train_device(X.ptr, min(n, SAMPLE), D, D, dsub, ITERS, 0,
                                                                            cb.ctypes.data_as(C.POINTER(C.c_float))))}, 1)["train"]
        made = []
        enc = measure(hip, {"encode": lambda: made.append(la.PqRows.from_device(X.ptr, n, D, D, cb, dsub))}, a.reps)["encode"]
        for b in made[:-1]:
            b.close()
        pq[dsub] = made[-1]
        notes.append(f"dsub = {dsub}: train ({min(n, SAMPLE)} rows, {ITERS} iterations, one timed call after warm-up) {train[0]:.1f} ms; encode median "
                     f"{enc[0]:.3f} ms, spread {enc[1]:.3f} ms (whole call: allocation, codebook upload, kernel, synchronisation); "
                     f"{n * pq[dsub].pitch() / 1e6:.1f} MB of codes ({pq[dsub].pitch()} B per row).")
    bits, mx4 = la.BitRows.from_device(X.ptr, n, D, D), la.Mx4Rows.from_device(X.ptr, n, D, D)
    i8 = la.BackendSearcher.build_device(la.BackendType.Hnsw, X.ptr, n, D, D, 16, 64, row_type=la.RowType.I8) if n <= a.i8_max_rows else None
    kmax = max(RECALL_FETCHES)
    keys, vals, counts = la.DeviceArray((nq, kmax), np.uint64), la.DeviceArray((nq, kmax), np.float32), la.DeviceArray(nq, np.uint32)
    objs = {"pq dsub 8": pq[8], "pq dsub 4": pq[4], "bits": bits, "mx4": mx4}
    legs = {name: (lambda o=o: o.search_batch_device(Q.ptr, nq, FETCH, keys.ptr, vals.ptr, counts.ptr)) for name, o in objs.items()}
    if i8:
        legs["int8 flat"] = lambda: i8.search_flat_batch_device(Q.ptr, nq, K, FETCH, keys.ptr, vals.ptr, counts.ptr)
    res = measure(hip, legs, a.reps)
    out.append(f"\n## {n} x {D}, nq = {nq}, fetch_k = {FETCH} ({a.reps} alternating runs)\n")
    out.append("| leg | median ms | spread ms | queries/s |\n|---|---|---|---|")
    for name, (med, spread) in res.items():
        out.append(f"| {name} | {med:.3f} | {spread:.3f} | {nq / med * 1e3:,.0f} |")
    out.append("\n" + "  \n".join(notes) + ("" if i8 else "  \nNo int8 twin at this size (--i8-max-rows)."))
    chk(L.leann_scan_topk_device(X.ptr, n, D, D, Q.ptr, nq, K, None, 0, keys.ptr, vals.ptr, counts.ptr, None))
    truth = keys.to_host().reshape(-1)[:nq * K].reshape(nq, K).copy()
    exact = la.ExactRows.from_device(X.ptr, n, D, D)
    out.append("\n| recall@10 against the f32 scan, refined on exact rows in HBM | " + " | ".join(f"fetch_k = {f}" for f in RECALL_FETCHES) + " |\n|---|"
               + "---|" * len(RECALL_FETCHES))
    for name, o in objs.items():
        cells = []
        for f in RECALL_FETCHES:
            o.search_refined_batch_device(exact, Q.ptr, nq, K, f, keys.ptr, vals.ptr, counts.ptr)
            cells.append(f"{recall(keys.to_host().reshape(-1)[:nq * K].reshape(nq, K), truth):.4f}")
        out.append(f"| {name} | " + " | ".join(cells) + " |")
    for o in (*objs.values(), exact, *([i8] if i8 else [])):
        o.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1000000, 10000000])
    ap.add_argument("--nq", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--i8-max-rows", type=int, default=10000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pq_rows.md"))
    a = ap.parse_args()
    import leann_rs_amd as la
    if la.device_count() < 1:
        sys.exit("pq_rows_bench: no HIP device visible")
    out = ["# PQ rows (scripts/pq_rows_bench.py; protocol in its docstring)"]
    for n in a.rows:
        for nq in a.nq:
            run_shape(la, la.lib(), a, n, nq, out)
            with open(a.out, "w") as f:  # after every shape: a later one that fails leaves the earlier ones
                f.write("\n".join(out) + "\n\nNot measured: kernel times on their own (rocprofv3), hardware counters (LDS bank conflicts of the "
                        "gather, whether LDS, the vector ALU or the L2 stream of codes binds score_pq_kernel), other widths than 768, recall "
                        "on a real embedding model.\n")


if __name__ == "__main__":
    main()
