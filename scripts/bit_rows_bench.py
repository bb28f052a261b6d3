#!/usr/bin/env python3
"""Sign-bit rows (csrc/scan_bits.hip) against the int8 flat search and the f32 exact scan; results go to
profiles/bit_rows.md.  Needs a GPU; fails without.  No thresholds: this prints what it measures.

    scripts/bit_rows_bench.py --rows 1000000 10000000 --nq 64 256

Per shape: synthetic rows n x 768 in HBM from leann_synth_rows_device (the f32 twin), their sign bits (leann_bit_rows_from_device,
timed: "pack"), an int8 HNSW handle built from the same rows (M = 16, efc = 64; only up to --i8-max-rows rows, the build being the
slowest step by far), nq queries.  Legs, for fetch_k = 40 and 1 000:
  bits        leann_bit_rows_search_batch_device, no bitmap
  int8 flat   leann_backend_search_flat_batch_device, top_k = 10, the same fetch_k
  f32 scan    leann_scan_topk_device over the f32 twin, top_k = 10 (once: it has no fetch_k)
Every call synchronises inside; a run is bracketed by device events on the null stream.  The legs alternate run by run: 3 warm-up runs
each, then --reps timed runs each; reported: median and spread (max - min).  These are WHOLE calls (query codes, score, select and
their synchronisations), not kernel times.
Recall@10 of leann_bit_rows_search_refined_batch_device against the f32 scan at fetch_k = 40, 100, 400, 1 000, without a centre and
with the column mean of the first 100 000 rows as the centre, the exact rows in HBM and (up to --host-max-rows rows) in pinned host
memory.  Synthetic clustered rows: no promise about a real embedding model."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, D, K, FETCHES, RECALL_FETCHES, BQ = 3, 768, 10, (40, 1000), (40, 100, 400, 1000), 64


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


def run_shape(la, hip, a, n, nq, out):
    L, chk = la.lib(), la._native.check
    X, Q = la.DeviceArray((n, D), np.float32), la.DeviceArray((nq, D), np.float32)
    chk(L.leann_synth_rows_device(0x5EED0001, D, D, 64, 4096, 1.0, 0, 0, n, X.ptr, None))
    chk(L.leann_synth_rows_device(0x5EED0001, D, D, 64, 4096, 1.0, 1, 0, nq, Q.ptr, None))
    la.sync()
    head = np.zeros((min(n, 100000), D), np.float32)
    chk(L.leann_device_download(head.ctypes.data, X.ptr, head.nbytes))
    centre = la.DeviceArray.from_host(head.mean(axis=0, dtype=np.float64).astype(np.float32))
    made = []
    pack = measure(hip, {"pack": lambda: made.append(la.BitRows.from_device(X.ptr, n, D, D))}, a.reps)["pack"]  # (allocation and close included)
    bits, bits_c = made[-1], la.BitRows.from_device(X.ptr, n, D, D, centre.ptr)
    for b in made[:-1]:
        b.close()
    i8 = la.BackendSearcher.build_device(la.BackendType.Hnsw, X.ptr, n, D, D, 16, 64, row_type=la.RowType.I8) if n <= a.i8_max_rows else None
    kmax = max(FETCHES)
    keys, vals, counts = la.DeviceArray((nq, kmax), np.uint64), la.DeviceArray((nq, kmax), np.float32), la.DeviceArray(nq, np.uint32)
    legs = {"f32 scan": lambda: chk(L.leann_scan_topk_device(X.ptr, n, D, D, Q.ptr, nq, K, None, 0, keys.ptr, vals.ptr, counts.ptr, None))}
    for f in FETCHES:
        legs[f"bits, fetch_k = {f}"] = lambda f=f: bits.search_batch_device(Q.ptr, nq, f, keys.ptr, vals.ptr, counts.ptr)
        if i8:
            legs[f"int8 flat, fetch_k = {f}"] = lambda f=f: i8.search_flat_batch_device(Q.ptr, nq, K, f, keys.ptr, vals.ptr, counts.ptr)
    res = measure(hip, legs, a.reps)
    out.append(f"\n## {n} x {D}, nq = {nq} ({a.reps} alternating runs)\n")
    out.append("| leg | median ms | spread ms | queries/s |\n|---|---|---|---|")
    for name, (med, spread) in res.items():
        out.append(f"| {name} | {med:.3f} | {spread:.3f} | {nq / med * 1e3:,.0f} |")
    tiles = (nq + BQ - 1) // BQ
    out.append(f"\npack: median {pack[0]:.3f} ms, spread {pack[1]:.3f} ms = {n * D * 4 / (pack[0] * 1e-3) / 1e12:.2f} TB/s of f32 read (whole "
               f"call: allocation, kernel, synchronisation).  Device memory of the object: {n * bits.pitch() / 1e6:.1f} MB ({bits.pitch()} B per "
               f"row; f32 rows {n * D * 4 / 1e6:.1f} MB, int8 rows {n * D / 1e6:.1f} MB).  A bits call sweeps {n * bits.pitch() * tiles / 1e9:.3f} GB "
               f"of rows and streams {n / 128 * BQ * 8 * bits.pitch() * tiles / 1e9:.2f} GB of query codes from L2; it issues "
               f"{2 * n * D * tiles * BQ / 1e12:.3f} TOP on the matrix cores." + ("" if i8 else "  No int8 twin at this size (--i8-max-rows)."))
    # recall of the refined search
    chk(L.leann_scan_topk_device(X.ptr, n, D, D, Q.ptr, nq, K, None, 0, keys.ptr, vals.ptr, counts.ptr, None))
    truth = keys.to_host().reshape(-1)[:nq * K].reshape(nq, K).copy()
    exact = {"HBM": la.ExactRows.from_device(X.ptr, n, D, D)}
    if n <= a.host_max_rows:
        exact["host"] = la.ExactRows.from_host(X.to_host(), placement="host")
    out.append("\n| recall@10 of the refined search | " + " | ".join(f"fetch_k = {f}" for f in RECALL_FETCHES) + " |\n|---|" + "---|" * len(RECALL_FETCHES))
    for place, rows in exact.items():
        for name, b in (("no centre", bits), ("centre = column mean", bits_c)):
            cells = []
            for f in RECALL_FETCHES:
                b.search_refined_batch_device(rows, Q.ptr, nq, K, f, keys.ptr, vals.ptr, counts.ptr)
                cells.append(f"{recall(keys.to_host().reshape(-1)[:nq * K].reshape(nq, K), truth):.4f}")
            out.append(f"| {name}, exact rows in {place} | " + " | ".join(cells) + " |")
    for o in (bits, bits_c, *exact.values(), *([i8] if i8 else [])):
        o.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1000000, 10000000])
    ap.add_argument("--nq", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--i8-max-rows", type=int, default=10000000)
    ap.add_argument("--host-max-rows", type=int, default=1000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bit_rows.md"))
    a = ap.parse_args()
    import leann_rs_amd as la
    if la.device_count() < 1:
        sys.exit("bit_rows_bench: no HIP device visible")
    out = ["# Sign-bit rows (scripts/bit_rows_bench.py; protocol in its docstring)"]
    for n in a.rows:
        for nq in a.nq:
            run_shape(la, la.lib(), a, n, nq, out)
            with open(a.out, "w") as f:  # after every shape: a later one that fails leaves the earlier ones
                f.write("\n".join(out) + "\n\nNot measured: kernel times on their own (rocprofv3), hardware counters (whether the matrix pipe, "
                        "the vector ALU's expansion, LDS or the L2 stream of query codes binds score_bits_mfma_kernel), other widths than "
                        "768, recall on a real embedding model.\n")


if __name__ == "__main__":
    main()
