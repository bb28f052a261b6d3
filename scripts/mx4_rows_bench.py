#!/usr/bin/env python3
"""MXFP4 rows (csrc/scan_mx4.hip) against sign-bit rows and the int8 flat search on the same rows in the same
process; results go to profiles/mx4_rows.md.  Needs a GPU; fails without.  No thresholds: this prints what it measures.

    scripts/mx4_rows_bench.py --rows 1000000 10000000 --nq 64 256

Per shape: synthetic rows n x 768 in HBM from leann_synth_rows_device (the f32 twin), their MXFP4 codes (leann_mx4_rows_from_device,
timed: "pack"), their sign bits, an int8 HNSW handle built from the same rows (M = 16, efc = 64; only up to --i8-max-rows rows, the
build being the slowest step by far), nq queries.  Legs, fetch_k = 40:
  mx4         leann_mx4_rows_search_batch_device, no bitmap
  bits        leann_bit_rows_search_batch_device, no bitmap
  int8 flat   leann_backend_search_flat_batch_device, top_k = 10
Every call synchronises inside; a run is bracketed by device events on the null stream.  The legs alternate run by run: 3 warm-up runs
each, then --reps timed runs each; reported: median and spread (max - min).  These are WHOLE calls (query codes, score, select and
their synchronisations), not kernel times.
Recall@10 against leann_scan_topk_device on the f32 twin at fetch_k = 40, 100, 400: leann_mx4_rows_search_refined_batch_device and
leann_bit_rows_search_refined_batch_device on the exact rows in HBM, and the int8 flat call's own answer (top_k = 10 of fetch_k by
the int8 distance).  Synthetic clustered rows: no promise about a real embedding model."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bit_rows_bench import BQ, D, K, measure, recall  # noqa: E402

FETCH, RECALL_FETCHES = 40, (40, 100, 400)


def run_shape(la, hip, a, n, nq, out):
    L, chk = la.lib(), la._native.check
    X, Q = la.DeviceArray((n, D), np.float32), la.DeviceArray((nq, D), np.float32)
    chk(L.leann_synth_rows_device(0x5EED0001, D, D, 64, 4096, 1.0, 0, 0, n, X.ptr, None))
    chk(L.leann_synth_rows_device(0x5EED0001, D, D, 64, 4096, 1.0, 1, 0, nq, Q.ptr, None))
    la.sync()
    made = []
    pack = measure(hip, {"pack": lambda: made.append(la.Mx4Rows.from_device(X.ptr, n, D, D))}, a.reps)["pack"]  # (allocation and close included)
    mx4, bits = made[-1], la.BitRows.from_device(X.ptr, n, D, D)
    for b in made[:-1]:
        b.close()
    i8 = la.BackendSearcher.build_device(la.BackendType.Hnsw, X.ptr, n, D, D, 16, 64, row_type=la.RowType.I8) if n <= a.i8_max_rows else None
    kmax = max(RECALL_FETCHES)
    keys, vals, counts = la.DeviceArray((nq, kmax), np.uint64), la.DeviceArray((nq, kmax), np.float32), la.DeviceArray(nq, np.uint32)
    legs = {"mx4": lambda: mx4.search_batch_device(Q.ptr, nq, FETCH, keys.ptr, vals.ptr, counts.ptr),
            "bits": lambda: bits.search_batch_device(Q.ptr, nq, FETCH, keys.ptr, vals.ptr, counts.ptr)}
    if i8:
        legs["int8 flat"] = lambda: i8.search_flat_batch_device(Q.ptr, nq, K, FETCH, keys.ptr, vals.ptr, counts.ptr)
    res = measure(hip, legs, a.reps)
    out.append(f"\n## {n} x {D}, nq = {nq}, fetch_k = {FETCH} ({a.reps} alternating runs)\n")
    out.append("| leg | median ms | spread ms | queries/s |\n|---|---|---|---|")
    for name, (med, spread) in res.items():
        out.append(f"| {name} | {med:.3f} | {spread:.3f} | {nq / med * 1e3:,.0f} |")
    row_bytes, tiles = 136 * ((D + 255) // 256), (nq + BQ - 1) // BQ
    out.append(f"\npack: median {pack[0]:.3f} ms, spread {pack[1]:.3f} ms = {n * D * 4 / (pack[0] * 1e-3) / 1e12:.2f} TB/s of f32 read (whole "
               f"call: allocation, kernel, synchronisation).  Device memory of the object: {n * row_bytes / 1e6:.1f} MB ({row_bytes} B per "
               f"row; sign bits {n * bits.pitch() / 1e6:.1f} MB, int8 rows {n * D / 1e6:.1f} MB, f32 rows {n * D * 4 / 1e6:.1f} MB).  An mx4 call "
               f"sweeps {n * row_bytes * tiles / 1e9:.3f} GB of rows and streams {n / 128 * BQ * 264 * ((D + 255) // 256) * tiles / 1e9:.2f} GB "
               f"of query codes from L2." + ("" if i8 else "  No int8 twin at this size (--i8-max-rows)."))
    chk(L.leann_scan_topk_device(X.ptr, n, D, D, Q.ptr, nq, K, None, 0, keys.ptr, vals.ptr, counts.ptr, None))
    truth = keys.to_host().reshape(-1)[:nq * K].reshape(nq, K).copy()
    exact = la.ExactRows.from_device(X.ptr, n, D, D)
    calls = {"mx4, refined on exact rows in HBM": lambda f: mx4.search_refined_batch_device(exact, Q.ptr, nq, K, f, keys.ptr, vals.ptr, counts.ptr),
             "bits (no centre), refined on exact rows in HBM": lambda f: bits.search_refined_batch_device(exact, Q.ptr, nq, K, f, keys.ptr, vals.ptr, counts.ptr)}
    if i8:
        calls["int8 flat (its own int8 distances)"] = lambda f: i8.search_flat_batch_device(Q.ptr, nq, K, f, keys.ptr, vals.ptr, counts.ptr)
    out.append("\n| recall@10 against the f32 scan | " + " | ".join(f"fetch_k = {f}" for f in RECALL_FETCHES) + " |\n|---|" + "---|" * len(RECALL_FETCHES))
    for name, call in calls.items():
        cells = []
        for f in RECALL_FETCHES:
            call(f)
            cells.append(f"{recall(keys.to_host().reshape(-1)[:nq * K].reshape(nq, K), truth):.4f}")
        out.append(f"| {name} | " + " | ".join(cells) + " |")
    for o in (mx4, bits, exact, *([i8] if i8 else [])):
        o.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1000000, 10000000])
    ap.add_argument("--nq", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--i8-max-rows", type=int, default=10000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx4_rows.md"))
    a = ap.parse_args()
    import leann_rs_amd as la
    if la.device_count() < 1:
        sys.exit("mx4_rows_bench: no HIP device visible")
    out = ["# MXFP4 rows (scripts/mx4_rows_bench.py; protocol in its docstring)"]
    for n in a.rows:
        for nq in a.nq:
            run_shape(la, la.lib(), a, n, nq, out)
            with open(a.out, "w") as f:  # after every shape: a later one that fails leaves the earlier ones
                f.write("\n".join(out) + "\n\nNot measured: kernel times on their own (rocprofv3), hardware counters (whether the matrix pipe, "
                        "LDS, HBM or the L2 stream of query codes binds score_mx4_mfma_kernel), other widths than 768, an FP6 or FP4 query at "
                        "the doubled instruction rate, recall on a real embedding model.\n")


if __name__ == "__main__":
    main()
