#!/usr/bin/env python3
"""Int8 rows under per-query filters (csrc/scan_lists_i8.hip): ONE leann_backend_search_flat_filtered_batch_device call
against the only way there was before it, nq single-query leann_backend_search_flat_batch_device calls, each under its own bitmap;
results go to profiles/flat_lists_i8.md.  Needs a GPU; fails without.  No thresholds: this prints what it measures.

    scripts/flat_lists_i8_bench.py --rows 1000000 10000000

Per shape: synthetic rows n x 768 in HBM, an int8 HNSW handle built from them (no leg reads the graph), 64 queries, k = 10,
fetch_k = 40, random bitmaps allowing about 1 % of the rows each.  Legs:
  a  single call / per-query loop   64 distinct bitmaps
  b  single call / per-query loop   8 distinct bitmaps, query i under bitmap i % 8 (the bitmap call cannot know they repeat)
  b  lists call                     leann_backend_search_flat_lists_batch_device over the 8 bitmaps' positions, q_list = i % 8
Before timing, every leg's keys, distance bits and counts are compared with the loop's.  Every call synchronises inside; a run is
bracketed by device events on the null stream.  The legs alternate run by run: 3 warm-up runs each, then --reps timed runs each;
reported: median and spread (max - min).  Algorithmic bytes: the allowed rows of every query, one 768-byte store row each — for the
lists call the rows of every list once, since its 8 queries are one tile that reads a chunk's rows once — against 8 TB/s, over the
WHOLE call (bitmap compaction, quantise, screen, select, rescore and their synchronisations).  Kernel times and hardware counters are
not read here."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.flat_i8_bench import measure  # noqa: E402

D, NQ, K, FETCH, PEAK = 768, 64, 10, 40, 8e12


def run_rows(la, hip, n, reps, out):
    L, chk = la.lib(), la._native.check
    X, Q = la.DeviceArray((n, D), np.float32), la.DeviceArray((NQ, D), np.float32)
    chk(L.leann_synth_rows_device(0x5EED0001, D, D, 64, 4096, 1.0, 0, 0, n, X.ptr, None))
    chk(L.leann_synth_rows_device(0x5EED0001, D, D, 64, 4096, 1.0, 1, 0, NQ, Q.ptr, None))
    la.sync()
    s = la.BackendSearcher.build_device(la.BackendType.Hnsw, X.ptr, n, D, D, 16, 64, row_type=la.RowType.I8)
    del X
    stride = (n + 7) // 8
    out.append(f"\n## {n} x {D}, nq = {NQ}, k = {K}, fetch_k = {FETCH}, about 1 % allowed per query ({reps} alternating runs)\n")
    out.append("| shape | leg | median ms | spread ms | share of 8 TB/s |\n|---|---|---|---|---|")
    for shape, distinct in (("a", NQ), ("b", 8)):
        rng = np.random.default_rng(distinct)
        bits = np.stack([rng.random(n) < 0.01 for _ in range(distinct)])
        bm = np.ascontiguousarray(np.packbits(bits, axis=-1, bitorder="little")[np.arange(NQ) % distinct])
        dbm = la.DeviceArray.from_host(bm)
        res = {}

        def outputs(name):
            res[name] = (la.DeviceArray((NQ, K), np.uint64), la.DeviceArray((NQ, K), np.float32), la.DeviceArray(NQ, np.uint32))
            return res[name]

        def loop(o=outputs("per-query loop")):
            for i in range(NQ):
                s.search_flat_batch_device(Q.ptr + 4 * D * i, 1, K, FETCH, o[0].ptr + 8 * K * i, o[1].ptr + 4 * K * i, o[2].ptr + 4 * i,
                                           d_allow=dbm.ptr + stride * i)

        def single(o=outputs("single call")):
            s.search_flat_filtered_batch_device(Q.ptr, NQ, K, FETCH, dbm.ptr, stride, o[0].ptr, o[1].ptr, o[2].ptr)

        legs = {"per-query loop": loop, "single call": single}
        if shape == "b":
            lists = [np.flatnonzero(b).astype(np.uint32) for b in bits]
            off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64)
            d_lists, ql = la.DeviceArray.from_host(np.concatenate(lists)), (np.arange(NQ) % 8).astype(np.uint32)

            def by_lists(o=outputs("lists call")):
                s.search_flat_lists_batch_device(Q.ptr, NQ, K, FETCH, off, d_lists.ptr, 8, ql, o[0].ptr, o[1].ptr, o[2].ptr)

            legs["lists call"] = by_lists
        for fn in legs.values():
            fn()
        la.sync()
        first = [a.to_host() for a in res["per-query loop"]]
        for name in legs:
            got = [a.to_host() for a in res[name]]
            assert all((g.view(np.uint32) == f.view(np.uint32)).all() for g, f in zip(got, first)), f"{name}: answers differ from the loop's"
        t, mark = measure(hip, legs, reps), len(out)
        row_bytes = int(bits[np.arange(NQ) % distinct].sum()) * D
        for name, (med, spread) in t.items():
            nbytes = int(bits.sum()) * D if name == "lists call" else row_bytes
            out.append(f"| {shape}: {distinct} distinct | {name} | {med:.3f} | {spread:.3f} | {nbytes / (med * 1e-3) / PEAK:.4f} |")
        (lm, ls), (sm, ss) = t["per-query loop"], t["single call"]
        out.append(f"| {shape} | loop / single call = {lm / sm:.2f} x; faster by more than both spreads together: "
                   f"{'yes' if lm - sm > ls + ss else 'no'} ({lm - sm:.3f} ms against {ls + ss:.3f} ms) | | | |")
        print("\n".join(out[mark:]), flush=True)
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1000000, 10000000])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flat_lists_i8.md"))
    a = ap.parse_args()
    import leann_rs_amd as la
    if la.device_count() < 1:
        sys.exit("flat_lists_i8_bench: no HIP device visible")
    out = ["# Int8 rows under per-query filters (scripts/flat_lists_i8_bench.py; protocol in its docstring)"]
    for n in a.rows:
        run_rows(la, la.lib(), n, a.reps, out)
        with open(a.out, "w") as f:  # after every shape: a later one that fails leaves the earlier ones
            f.write("\n".join(out) + "\n\nNot measured: score_lists_i8_kernel's own time and its share of the HBM peak (rocprofv3), hardware "
                    "counters (LDS conflicts, which of the gather, LDS and the vector ALU binds it), lists shared by 32 or more queries "
                    "against the MFMA screen, other widths than 768, fetch_k other than 40.\n")


if __name__ == "__main__":
    main()
