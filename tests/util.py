import numpy as np

# synthetic-set defaults: seed, r, clusters, sigma
SEED = 0x5EED0001
GEN = dict(r=64, n_clusters=4096, sigma=1.0)


def synth(po, n, d, stream=0, i0=0, r=64, n_clusters=256, sigma=1.0, seed=SEED):
    return po.gen_rows(seed, d, r, n_clusters, sigma, stream, i0, n)


class HipStreams:
    """n non-blocking HIP streams (hipStreamCreateWithFlags(.., hipStreamNonBlocking)) for the stream= parameters of backend.py, made
    with ctypes on the HIP runtime libleann_hip.so links — symbols are looked up through the library's own handle, so no second
    runtime is loaded and no torch is needed.  streams[i] is the integer those parameters accept; `with HipStreams(la, 8) as st:`
    destroys them.  call(name, ...) is any runtime function of SIGNATURES, checked: a non-zero hipError_t raises."""
    import ctypes as _C
    NON_BLOCKING = 1  # hipStreamNonBlocking
    D2H, D2D = 2, 3   # hipMemcpyDeviceToHost, hipMemcpyDeviceToDevice
    _vp, _vpp = _C.c_void_p, _C.POINTER(_C.c_void_p)
    SIGNATURES = {
        "hipStreamCreateWithFlags": [_vpp, _C.c_uint],
        "hipStreamDestroy": [_vp],
        "hipStreamSynchronize": [_vp],
        "hipMemcpyAsync": [_vp, _vp, _C.c_size_t, _C.c_int, _vp],
        "hipEventCreateWithFlags": [_vpp, _C.c_uint],
        "hipEventDestroy": [_vp],
        "hipEventRecord": [_vp, _vp],
        "hipStreamWaitEvent": [_vp, _vp, _C.c_uint],
        "hipStreamBeginCapture": [_vp, _C.c_int],
        "hipStreamEndCapture": [_vp, _vpp],
        "hipGraphInstantiate": [_vpp, _vp, _vpp, _C.c_char_p, _C.c_size_t],
        "hipGraphLaunch": [_vp, _vp],
        "hipGraphExecDestroy": [_vp],
        "hipGraphDestroy": [_vp],
    }

    def __init__(self, la, n):
        self._rt = la.lib()
        self._rt.hipGetErrorString.restype = self._C.c_char_p
        self._rt.hipGetErrorString.argtypes = [self._C.c_int]
        self.streams = []
        for _ in range(n):
            self.streams.append(self.create("hipStreamCreateWithFlags", self.NON_BLOCKING))

    def call(self, name, *args):
        f = getattr(self._rt, name)
        f.restype, f.argtypes = self._C.c_int, self.SIGNATURES[name]
        rc = f(*args)
        if rc != 0:
            raise RuntimeError(f"{name}: hipError {rc}: {self._rt.hipGetErrorString(rc).decode('utf-8', 'replace')}")

    def create(self, name, *args):
        """a runtime function whose first parameter is the address the new handle is written to; returns the handle as an integer"""
        out = self._C.c_void_p()
        self.call(name, self._C.byref(out), *args)
        return out.value

    def synchronize(self, stream):
        self.call("hipStreamSynchronize", stream)

    def copy_async(self, dst, src, nbytes, kind, stream):
        self.call("hipMemcpyAsync", dst, src, nbytes, kind, stream)

    def __len__(self):
        return len(self.streams)

    def __iter__(self):
        return iter(self.streams)

    def __getitem__(self, i):
        return self.streams[i]

    def close(self):
        for s in self.streams:
            self.call("hipStreamDestroy", s)
        self.streams = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def recall_at_k(found, truth):
    k = truth.shape[1]
    hits = 0
    for f, t in zip(found, truth):
        hits += len(set(int(x) for x in f[:k]) & set(int(x) for x in t))
    return hits / (len(truth) * k)


def traced_graph(name="traced_graph_64.json"):
    """tests/golden/traced_graph_64.json (hand-built 64-node graph) or traced_graph_400.json (400 nodes, three levels, duplicated
    vectors) as arrays + the independently traced expectations"""
    import json, os
    fx = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)))
    X = np.array(fx["vectors"], np.float32)
    levels = np.array(fx["levels"], np.uint8)
    upper_off = np.concatenate([[0], np.cumsum(levels)[:-1]]).astype(np.uint32)
    adj0 = np.array(fx["adj0"], np.uint32)
    adjU = np.array(fx["adjU"], np.uint32)
    return fx, X, levels, upper_off, adj0, adjU


def write_gx1(path, kind, X, M, M0, max_level, entry, levels, upper_off, adj0, adjU, efc=64, alpha=1.2):
    """a version-1 LEANNGX1 index file (csrc/indexfile.hip) written from numpy arrays; returns the header bytes"""
    import struct
    X = np.ascontiguousarray(X, np.float32)
    n, d = X.shape
    adjU = np.ascontiguousarray(adjU, np.uint32).reshape(-1, M) if np.size(adjU) else np.zeros((0, M), np.uint32)
    hd = struct.pack("<8sIIQIIIIIIfIQI60x", b"LEANNGX1", 1, kind, n, d, M, M0, max_level, entry, efc, alpha, 0, adjU.shape[0], 0)
    assert len(hd) == 128
    with open(path, "wb") as f:
        f.write(hd)
        f.write(np.ascontiguousarray(levels, np.uint8).tobytes())
        f.write(np.ascontiguousarray(upper_off, np.uint32).tobytes())
        f.write(np.ascontiguousarray(adj0, np.uint32).tobytes())
        f.write(adjU.tobytes())
        f.write(X.tobytes())
    return hd


def write_gx2(path, kind, d, M, M0, max_level, entry, levels, upper_off, adj0, adjU, rows, feat_h, W, efc=64, alpha=1.2):
    """a version-2 LEANNGX1 index file (recompute-on: no vectors) written from numpy arrays: rows = uint8 [n, row_bytes] holding
    feat_h bf16 features, the f32 norm and padding; W = the encoder weights as f32 [feat_h, d]; returns the header bytes"""
    import struct
    rows = np.ascontiguousarray(rows, np.uint8)
    n, row_bytes = rows.shape
    W = np.ascontiguousarray(W, np.float32)
    assert W.shape == (feat_h, d) and row_bytes >= 2 * feat_h + 4 and row_bytes % 8 == 0
    adjU = np.ascontiguousarray(adjU, np.uint32).reshape(-1, M) if np.size(adjU) else np.zeros((0, M), np.uint32)
    hd = struct.pack("<8sIIQIIIIIIfIQI60x", b"LEANNGX1", 2, kind, n, d, M, M0, max_level, entry, efc, alpha, feat_h, adjU.shape[0], row_bytes)
    assert len(hd) == 128
    with open(path, "wb") as f:
        f.write(hd)
        f.write(np.ascontiguousarray(levels, np.uint8).tobytes())
        f.write(np.ascontiguousarray(upper_off, np.uint32).tobytes())
        f.write(np.ascontiguousarray(adj0, np.uint32).tobytes())
        f.write(adjU.tobytes())
        f.write(rows.tobytes())
        f.write(W.tobytes())
    return hd
