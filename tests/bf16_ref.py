"""bf16 rows in numpy, for the tests of the bf16 row type: r = f32 -> bf16, round to nearest even with NaN staying NaN (the arithmetic
of csrc/bf16.h, restated independently), w = the exact widening, and a writer of version-3 index files."""
import struct

import numpy as np


def round_bf16(x):
    """r(x): uint16 array of the shape of x"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    rne = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, (u >> 16) | 0x40, rne).astype(np.uint16)


def widen(b):
    """w(b): float32 array of the shape of b, exact"""
    return (np.ascontiguousarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)


def rounded(x):
    """Xr = w(r(X))"""
    return widen(round_bf16(x))


def write_gx3(path, kind, rows_bf16, M, M0, max_level, entry, levels, upper_off, adj0, adjU, efc=64, alpha=1.2):
    """a version-3 LEANNGX1 index file (csrc/indexfile.hip): the header and graph arrays of version 1, then unpadded bf16 rows
    [n x d] in element order; returns the header bytes"""
    B = np.ascontiguousarray(rows_bf16, np.uint16)
    n, d = B.shape
    adjU = np.ascontiguousarray(adjU, np.uint32).reshape(-1, M) if np.size(adjU) else np.zeros((0, M), np.uint32)
    hd = struct.pack("<8sIIQIIIIIIfIQI60x", b"LEANNGX1", 3, kind, n, d, M, M0, max_level, entry, efc, alpha, 0, adjU.shape[0], 0)
    assert len(hd) == 128
    with open(path, "wb") as f:
        f.write(hd)
        f.write(np.ascontiguousarray(levels, np.uint8).tobytes())
        f.write(np.ascontiguousarray(upper_off, np.uint32).tobytes())
        f.write(np.ascontiguousarray(adj0, np.uint32).tobytes())
        f.write(adjU.tobytes())
        f.write(B.tobytes())
    return hd
