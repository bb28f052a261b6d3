"""Helper of tests/test_gpu_streams.py::test_hip_graph_replay_of_eight_forked_calls (not a test; run as `python stream_graph_child.py
OUT.npz` in a process of its own, so that a failed capture leaves nothing behind in the pytest process).

On a 20 000 x 128 HNSW handle built on the device: every stream is warmed with one call and the device synchronised; then
fork -> 8 calls of 64 queries on 8 non-blocking streams -> join is captured into a HIP graph (the sequence of bench.py's small-batch
leg, through the HIP runtime directly: no torch) and replayed three times.  Before each replay the CONTENTS of the eight query buffers
are overwritten with eight other query sets, the pointers stay; after each replay all eight results are copied out.  The same 24
(set, buffer) calls then run uncaptured on the null stream.  Both sets of answers, the query sets and the exported graph go into
OUT.npz.  Any HIP or library error ends the process with a traceback and a non-zero status."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "oracle"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

N, D, M, NQ, K, EF, S, REPLAYS = 20_000, 128, 16, 64, 10, 64, 8, 3
CAPTURE_MODE_GLOBAL = 0   # hipStreamCaptureModeGlobal: an allocation or a synchronisation by any thread invalidates the capture
EVENT_DISABLE_TIMING = 2  # hipEventDisableTiming


def main(out_path):
    import leann_rs_amd as la
    import pyoracle as po
    from util import HipStreams, synth

    assert la.device_count() >= 1, "no HIP device visible"
    X = synth(po, N, D)
    dX = la.DeviceArray.from_host(X)
    s = la.BackendSearcher.build_device(la.BackendType.Hnsw, dX.ptr, N, D, D, M, 64)
    g = s.graph_export()
    Q = np.stack([synth(po, NQ, D, stream=1, i0=1000 * j) for j in range(REPLAYS * S)])
    sets = np.arange(REPLAYS * S).reshape(REPLAYS, S)  # replay r, buffer b runs set 8 r + b
    dQ = [la.DeviceArray((NQ, D), np.float32) for _ in range(S)]
    dk = [la.DeviceArray((NQ, K), np.uint64) for _ in range(S)]
    dd = [la.DeviceArray((NQ, K), np.float32) for _ in range(S)]
    dc = [la.DeviceArray(NQ, np.uint32) for _ in range(S)]
    dst = [la.DeviceArray((NQ, 4), np.uint32) for _ in range(S)]
    res = {w: {n_: np.zeros((REPLAYS, S, NQ) + tail, dt) for n_, tail, dt in (("keys", (K,), np.uint64), ("dist_bits", (K,), np.uint32),
                                                                             ("counts", (), np.uint32), ("stats", (4,), np.uint32))}
           for w in ("graph", "plain")}

    def call(b, stream):
        s.search_batch_device(dQ[b].ptr, NQ, K, EF, dk[b].ptr, dd[b].ptr, dc[b].ptr, d_stats=dst[b].ptr, stream=stream)

    def load(r):
        """set sets[r, b] into query buffer b, a pattern no answer holds into every output; all of it done before returning"""
        for b in range(S):
            dQ[b].upload(Q[sets[r, b]])
            dk[b].upload(np.full((NQ, K), 0xABABABABABABABAB, np.uint64))
            dd[b].upload(np.full((NQ, K), 0xABABABAB, np.uint32).view(np.float32))
            dc[b].upload(np.full(NQ, 0xABABABAB, np.uint32))
            dst[b].upload(np.full((NQ, 4), 0xABABABAB, np.uint32))
        la.sync()

    def store(which, r):
        for b in range(S):
            res[which]["keys"][r, b] = dk[b].to_host()
            res[which]["dist_bits"][r, b] = dd[b].to_host().view(np.uint32)
            res[which]["counts"][r, b] = dc[b].to_host()
            res[which]["stats"][r, b] = dst[b].to_host()

    with HipStreams(la, S + 1) as hip:
        sts, cap = hip.streams[:S], hip.streams[S]
        fork = hip.create("hipEventCreateWithFlags", EVENT_DISABLE_TIMING)
        joins = [hip.create("hipEventCreateWithFlags", EVENT_DISABLE_TIMING) for _ in range(S)]
        load(0)
        for b in range(S):  # warm: after this a call allocates nothing
            call(b, sts[b])
        la.sync()
        hip.call("hipStreamBeginCapture", cap, CAPTURE_MODE_GLOBAL)
        hip.call("hipEventRecord", fork, cap)
        for b in range(S):  # fork ...
            hip.call("hipStreamWaitEvent", sts[b], fork, 0)
        for b in range(S):
            call(b, sts[b])
        for b in range(S):  # ... join
            hip.call("hipEventRecord", joins[b], sts[b])
            hip.call("hipStreamWaitEvent", cap, joins[b], 0)
        graph = C.c_void_p()
        hip.call("hipStreamEndCapture", cap, C.byref(graph))
        assert graph.value, "hipStreamEndCapture returned no graph"
        exe = hip.create("hipGraphInstantiate", graph, None, None, 0)
        print(f"captured {S} calls of {NQ} queries on {S} streams", flush=True)
        for r in range(REPLAYS):
            load(r)
            hip.call("hipGraphLaunch", exe, cap)
            hip.synchronize(cap)
            la.sync()
            store("graph", r)
            print(f"replay {r} done", flush=True)
        hip.call("hipGraphExecDestroy", exe)
        hip.call("hipGraphDestroy", graph)
        for e in [fork] + joins:
            hip.call("hipEventDestroy", e)
    for r in range(REPLAYS):  # the same (set, buffer) calls, uncaptured, on the null stream
        load(r)
        for b in range(S):
            call(b, None)
        la.sync()
        store("plain", r)
    s.close()
    np.savez(out_path, queries=Q, sets=sets, M=g["M"], M0=g["M0"], max_level=g["max_level"], entry=g["entry"], levels=g["levels"],
             upper_off=g["upper_off"], adj0=g["adj0"], adjU=g["adjU"],
             **{f"{w}_{n_}": a for w, d_ in res.items() for n_, a in d_.items()})
    print("child ok", flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
