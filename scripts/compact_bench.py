"""Time of leann_backend_compact on one GPU: n x d f32 rows (default 10M x 768), a fraction removed (default 30 %), consolidated.

The library times its own phases with device events when LEANN_LOG=info (csrc/compact.hip: the "compact:" line — list remap, row
gather, plane re-cut); this script makes the handle, runs one warm-up compaction and `--repeats` measured ones (each result is closed
before the next: the allocator sees the same state every time), and reports the median of each phase next to the bytes moved,
(live x row_bytes + lists) x 2, and the share of a 6.3 TB/s copy that is.  The wall time of the whole call (host map, allocations,
uploads, the phases) is reported beside them.

    python scripts/compact_bench.py [--n 10000000] [--d 768] [--degree 8] [--complexity 32] [--fraction 0.3] [--out FILE]

The graph is built by the device builder with a small degree: compaction does not care how good the graph is, only how wide."""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time

os.environ["LEANN_LOG"] = "info"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import leann_rs_amd as la  # noqa: E402

COPY_PEAK = 6.3e12  # bytes/s a device-to-device copy reaches on this part
LINE = re.compile(r"compact: (\d+) of (\d+) positions kept; lists ([\d.]+) ms \(([\d.]+) GB moved\), rows ([\d.]+) ms \(([\d.]+) GB moved, "
                  r"(\d+) GB/s\), planes ([\d.]+) ms( \(none cut\))?")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--degree", type=int, default=8)
    ap.add_argument("--complexity", type=int, default=32)
    ap.add_argument("--fraction", type=float, default=0.30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    log = tempfile.TemporaryFile(mode="w+b")
    sys.stderr.flush()
    keep = os.dup(2)
    os.dup2(log.fileno(), 2)  # the library logs to stderr
    try:
        L = la.lib()
        rows = la.DeviceArray((a.n, a.d), np.float32)
        la._native.check(L.leann_synth_rows_device(0x5EED0001, a.d, a.d, 64, 4096, 1.0, 0, 0, a.n, rows.ptr, None))
        la.sync()
        t = time.time()
        s = la.BackendSearcher.build_device(la.BackendType.Hnsw, rows.ptr, a.n, a.d, a.d, a.degree, a.complexity)
        build_s = time.time() - t
        rng = np.random.default_rng(1)
        gone = np.flatnonzero(rng.random(a.n) < a.fraction).astype(np.uint64)
        s.remove(gone)
        t = time.time()
        s.consolidate()
        consolidate_s = time.time() - t
        walls = []
        for _ in range(a.repeats + 1):
            t = time.time()
            c, m = s.compact()
            walls.append(time.time() - t)
            assert c.len() == a.n - len(gone) == len(m)
            c.close()
        s.close()
    finally:
        os.dup2(keep, 2)
    log.seek(0)
    text = log.read().decode("utf-8", "replace")
    sys.stderr.write(text)
    runs = [mt.groups() for mt in map(LINE.search, text.splitlines()) if mt][1:]  # the first is the warm-up
    if len(runs) != a.repeats:
        raise SystemExit(f"expected {a.repeats} timing lines, found {len(runs)}")
    med = lambda i: statistics.median(float(r[i]) for r in runs)  # noqa: E731
    lists_ms, rows_ms, planes_ms = med(2), med(4), med(7)
    list_gb, row_gb = float(runs[0][3]), float(runs[0][5])
    out = dict(n=a.n, d=a.d, degree=a.degree, removed=int(len(gone)), live=int(runs[0][0]), repeats=a.repeats,
               build_s=round(build_s, 2), consolidate_s=round(consolidate_s, 2),
               rows_ms=rows_ms, rows_gb_moved=row_gb, rows_gb_per_s=round(row_gb / (rows_ms * 1e-3), 1),
               rows_share_of_copy_peak=round(row_gb * 1e9 / (rows_ms * 1e-3) / COPY_PEAK, 3),
               rows_ms_all=[float(r[4]) for r in runs],
               lists_ms=lists_ms, lists_gb_moved=list_gb, lists_ms_all=[float(r[2]) for r in runs],
               planes_ms=planes_ms, planes_cut=runs[0][8] is None, planes_ms_all=[float(r[7]) for r in runs],
               call_wall_s=round(statistics.median(walls[1:]), 3), call_wall_s_all=[round(w, 3) for w in walls[1:]])
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
