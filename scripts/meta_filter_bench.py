#!/usr/bin/env python3
"""What registering a NEW metadata filter costs, two ways (results in profiles/meta_filter.md).  Needs a GPU; fails without.

Part A, through the C ABI, at --rows synthetic passages with three fields (lines: number, type: 3 distinct strings, source: rows / 8
distinct strings): the one-off column build per field (leann_meta_add_column: dictionary sort + upload), the device memory per
column, and per filter  compile (host clock around leann_meta_eval_device, which compiles and enqueues without waiting), the device
window (device events around the same call: it holds the host's compile AND the kernel) and the whole registration
(leann_backend_filter_create_meta: evaluate, AND the live mask, compact; host clock, it ends in a synchronise).  The kernel's own time
comes from a second run under `rocprofv3 --kernel-trace`, folded in afterwards with --fold-trace RESULT.json TRACE.csv: per filter
the median over the --reps dispatches of meta_eval_kernel.  Kernel bytes are counted from the program: per row 1 B of tag per column
touched + 8 B per NUMBER row whose number is tested + 4 B per STRING row whose code is tested + 1 bit out; the share of the HBM peak
is those bytes over the kernel time over 8.0 TB/s.

Part B, through the C++ host (--cli-rows passages, 0 = skip): `leann build`, then `leann search -f F --device-filter` with LEANN_LOG=debug
once as it is and once with LEANN_META_DEVICE=0 — the second is the parent commit's per-passage loop, unchanged — reading the times
IndexSearcher logs.  The device path's first filter on a field includes that field's one pass over the passages."""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12


def digits(values, width):
    """[n x width] ASCII decimal digits of `values`, zero padded"""
    out = np.empty((len(values), width), np.uint8)
    v = values.astype(np.uint64)
    for j in range(width - 1, -1, -1):
        out[:, j] = (v % 10) + 48
        v //= 10
    return out


class Events:
    def __init__(self, la):
        self.rt = la.lib()
        self.vp = C.c_void_p

    def create(self):
        e = self.vp()
        assert self.rt.hipEventCreate(C.byref(e)) == 0
        return e

    def record(self, e):
        assert self.rt.hipEventRecord(e, None) == 0

    def elapsed_ms(self, a, b):
        assert self.rt.hipEventSynchronize(b) == 0
        ms = C.c_float(0)
        assert self.rt.hipEventElapsedTime(C.byref(ms), a, b) == 0
        return ms.value


def part_a(la, n, reps, out):
    rng = np.random.default_rng(1)
    ev = Events(la)
    lines = rng.integers(0, 200, n).astype(np.float64)
    types = [b"code", b"text", b"doc"]
    tsel = rng.integers(0, 3, n)
    m = la.MetaColumns(n)
    build = {}
    t = time.perf_counter()
    m.add_column("lines", np.full(n, 4, np.uint8), lines)
    build["lines"] = time.perf_counter() - t
    lens = np.array([len(x) for x in types], np.uint64)[tsel]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    blob = b"".join(types[i] for i in tsel.tolist())
    t = time.perf_counter()
    m.add_column("type", np.full(n, 5, np.uint8), None, blob, off)
    build["type"] = time.perf_counter() - t
    src = np.concatenate([np.frombuffer(b"/p/", np.uint8)[None, :].repeat(n, 0), digits(rng.integers(0, max(n // 8, 1), n), 8),
                          np.frombuffer(b".rs", np.uint8)[None, :].repeat(n, 0)], axis=1)
    t = time.perf_counter()
    m.add_column("source", np.full(n, 5, np.uint8), None, src.tobytes(), (np.arange(n + 1, dtype=np.uint64) * np.uint64(src.shape[1])))
    build["source"] = time.perf_counter() - t
    out["column_build_s"] = build
    out["column_device_bytes"] = {"lines": n * 9, "type": n * 5, "source": n * 5}
    # a handle of the same length to register on: tiny rows, the graph is not what is measured
    d = 8
    dX = la.DeviceArray.from_host(rng.standard_normal((n, d)).astype(np.float32))
    s = la.BackendSearcher.build_device(la.BackendType.Hnsw, dX.ptr, n, d, d, 4, 16)
    nbytes = (n + 7) // 8
    d_bm = la.DeviceArray(nbytes, np.uint8)
    filters = [("lines>50", n * (1 + 8)), ("type=code", n * (1 + 4)), ("lines>50 AND type=code AND source^/p/0000", n * (1 + 8 + 1 + 4 + 1 + 4)),
               ("source~77.rs", n * (1 + 4)), ("type in [code,doc] OR lines<=20", n * (1 + 4 + 1 + 8))]
    e0, e1 = ev.create(), ev.create()
    rows = []
    for text, col_bytes in filters:
        m.eval_device(text, d_bm.ptr)  # warm-up: code object, the stream's scratch block
        la.sync()
        comp, kern = [], []
        for _ in range(reps):
            ev.record(e0)
            t = time.perf_counter()
            m.eval_device(text, d_bm.ptr)
            comp.append(time.perf_counter() - t)
            ev.record(e1)
            kern.append(ev.elapsed_ms(e0, e1) * 1e-3)
        reg = []
        for _ in range(max(reps // 4, 3)):
            t = time.perf_counter()
            f = s.register_meta_filter(m, text)
            reg.append(time.perf_counter() - t)
            allowed = f.count()
            f.close()
        rows.append(dict(filter=text, allowed=allowed, compile_enqueue_ms=1e3 * float(np.median(comp)), device_window_ms=1e3 * float(np.median(kern)),
                         device_window_ms_min_max=[1e3 * min(kern), 1e3 * max(kern)], kernel_bytes=col_bytes + nbytes,
                         register_total_ms=1e3 * float(np.median(reg)), dispatches=1 + reps + len(reg)))
    out["filters"] = rows
    m.close()
    s.close()


def part_b(n, out):
    exe = os.path.join(ROOT, "leann-rs_amd", "host", "leann")
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "docs.jsonl"), "w") as f:
            for i in range(n):
                f.write(json.dumps(dict(id=str(i + 1), text=f"passage {i} topic {i % 97}",
                                        metadata=dict(source=f"/p/{i % (n // 8 + 1):08d}.rs", lines=i % 200, type=["code", "text", "doc"][i % 3]))) + "\n")
        t = time.perf_counter()
        subprocess.run([exe, "build", "--index-dir", os.path.join(d, "idx"), "--passages-jsonl", os.path.join(d, "docs.jsonl"), "--dimensions", "32",
                        "--graph-degree", "8", "--complexity", "32"], check=True, capture_output=True)
        out["cli_build_s"] = time.perf_counter() - t
        res = {}
        for flt in ("lines>50", "lines>50 AND type=code"):
            for knob in ("1", "0"):
                env = dict(os.environ, LEANN_LOG="debug", LEANN_META_DEVICE=knob)
                r = subprocess.run([exe, "search", "passage topic 5 and more words here", "-i", os.path.join(d, "idx"), "--top-k", "5", "--format", "json",
                                    "--auto-hybrid", "false", "-f", flt, "--device-filter"], capture_output=True, text=True, env=env, check=True)
                ms = re.search(r"registered in ([0-9.]+) ms", r.stderr)
                res[f"{flt} | {'device (first use: includes the column pass)' if knob == '1' else 'host pass'}"] = float(ms.group(1)) if ms else None
        out["cli_register_ms"] = res


def fold_trace(result_file, trace_csv):
    """kernel times of meta_eval_kernel from a rocprofv3 kernel trace of the same command line, in dispatch order"""
    import csv
    out = json.load(open(result_file))
    with open(trace_csv) as f:
        rows = [r for r in csv.DictReader(f) if "meta_eval_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dur = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9 for r in rows]
    at = 0
    for flt in out["filters"]:
        mine = dur[at + 1: at + 1 + out["reps"]]  # behind the warm-up, before the registrations
        at += flt["dispatches"]
        k = float(np.median(mine))
        flt.update(kernel_ms=1e3 * k, kernel_ms_min_max=[1e3 * min(mine), 1e3 * max(mine)], kernel_GBps=flt["kernel_bytes"] / k / 1e9,
                   share_of_hbm_peak=flt["kernel_bytes"] / k / HBM_PEAK)
    assert at == len(dur), (at, len(dur))
    print(json.dumps(out, indent=1))


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--fold-trace":
        return fold_trace(sys.argv[2], sys.argv[3])
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cli-rows", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import leann_rs_amd as la
    if la.device_count() < 1:
        raise SystemExit("meta_filter_bench: no HIP device visible")
    out = dict(rows=a.rows, reps=a.reps)
    part_a(la, a.rows, a.reps, out)
    if a.cli_rows:
        out["cli_rows"] = a.cli_rows
        part_b(a.cli_rows, out)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
