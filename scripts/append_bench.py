"""Time of leann_backend_append_device on one GPU against its file twin (leann_backend_add + reopening the file).

An n x d HNSW handle (default 1M x 768, M = 32) is built on the device once; then, for every size in --add (default 1 000 and
100 000 rows) and --repeats times each:

  handle   s.append_device(new rows)            device events on the null stream around the call + wall time; the result is closed
                                                before the next repeat
  file     BackendBuilder.add_to_index(rows)    wall time of the call on a fresh copy of the saved index, plus the wall time of
           + HnswSearcher.load                  opening the file it wrote (what a server does next); --no-file-twin skips it

and prints one JSON line (medians and every figure).  The rows are the synthetic set of bench.py; the appended rows continue it.

    python scripts/append_bench.py [--n 1000000] [--d 768] [--degree 32] [--complexity 64] [--add 1000,100000] [--repeats 3] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import leann_rs_amd as la  # noqa: E402


class Events:
    """two HIP events on the null stream, through the runtime the library links"""

    def __init__(self):
        self.rt = la.lib()
        self.a, self.b = C.c_void_p(), C.c_void_p()
        for e in (self.a, self.b):
            self._call("hipEventCreate", [C.POINTER(C.c_void_p)], C.byref(e))

    def _call(self, name, argtypes, *args):
        f = getattr(self.rt, name)
        f.restype, f.argtypes = C.c_int, argtypes
        rc = f(*args)
        if rc != 0:
            raise RuntimeError(f"{name}: hipError {rc}")

    def start(self):
        self._call("hipEventRecord", [C.c_void_p, C.c_void_p], self.a, None)

    def stop_ms(self):
        self._call("hipEventRecord", [C.c_void_p, C.c_void_p], self.b, None)
        self._call("hipEventSynchronize", [C.c_void_p], self.b)
        ms = C.c_float(0)
        self._call("hipEventElapsedTime", [C.POINTER(C.c_float), C.c_void_p, C.c_void_p], C.byref(ms), self.a, self.b)
        return float(ms.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--degree", type=int, default=32)
    ap.add_argument("--complexity", type=int, default=64)
    ap.add_argument("--add", default="1000,100000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-file-twin", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    adds = [int(x) for x in a.add.split(",")]
    L, chk = la.lib(), la._native.check
    total = a.n + max(adds)
    rows = la.DeviceArray((total, a.d), np.float32)
    chk(L.leann_synth_rows_device(0x5EED0001, a.d, a.d, 64, 4096, 1.0, 0, 0, total, rows.ptr, None))
    la.sync()
    t = time.time()
    s = la.BackendSearcher.build_device(la.BackendType.Hnsw, rows.ptr, a.n, a.d, a.d, a.degree, a.complexity)
    build_s = time.time() - t
    new_ptr = rows.ptr + a.n * a.d * 4
    ev = Events()
    out = dict(n=a.n, d=a.d, degree=a.degree, complexity=a.complexity, repeats=a.repeats, build_s=round(build_s, 2), sizes={})
    for m in adds:
        dev_ms, wall_s = [], []
        for _ in range(a.repeats + 1):  # the first is the warm-up
            la.sync()
            t = time.time()
            ev.start()
            r = s.append_device(new_ptr, m, a.d)
            dev_ms.append(ev.stop_ms())
            wall_s.append(time.time() - t)
            assert r.len() == a.n + m
            r.close()
        out["sizes"][str(m)] = dict(handle_device_ms=round(statistics.median(dev_ms[1:]), 2), handle_wall_s=round(statistics.median(wall_s[1:]), 4),
                                    handle_device_ms_all=[round(x, 2) for x in dev_ms[1:]], handle_wall_s_all=[round(x, 4) for x in wall_s[1:]])
    if not a.no_file_twin:
        host = np.empty((max(adds), a.d), np.float32)
        chk(L.leann_device_download(host.ctypes.data, new_ptr, host.nbytes))
        with tempfile.TemporaryDirectory() as tmp:
            base, work = os.path.join(tmp, "base"), os.path.join(tmp, "work")
            os.mkdir(base)
            s.save(os.path.join(base, "documents.leann"))
            b = la.BackendBuilder(la.BackendType.Hnsw)
            for m in adds:
                add_s, open_s = [], []
                for _ in range(a.repeats):
                    shutil.rmtree(work, ignore_errors=True)
                    shutil.copytree(base, work)
                    stem = os.path.join(work, "documents.leann")
                    t = time.time()
                    b.add_to_index(host[:m], stem, a.d, a.n)
                    add_s.append(time.time() - t)
                    t = time.time()
                    o = la.HnswSearcher.load(stem, a.d)
                    open_s.append(time.time() - t)
                    assert o.len() == a.n + m
                    o.close()
                out["sizes"][str(m)].update(file_add_s=round(statistics.median(add_s), 3), file_reopen_s=round(statistics.median(open_s), 3),
                                            file_add_s_all=[round(x, 3) for x in add_s], file_reopen_s_all=[round(x, 3) for x in open_s])
    s.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
