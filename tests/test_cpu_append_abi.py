"""CPU suite: leann_backend_append / leann_backend_append_device are exported and bound, and their argument checks answer before any
device work (include/leann_backend.h "appending to a handle"): no handle can exist without a device, so what is reachable here is the
NULL handle and the NULL result, whatever the other arguments say."""
import ctypes as C

import numpy as np

INVALID = 1


def test_symbols_resolve_and_are_bound(la):
    L = la.lib()
    for name in ("leann_backend_append", "leann_backend_append_device"):
        assert hasattr(L, name) and name in la._native.SIGNATURES
    assert callable(la.BackendSearcher.append) and callable(la.BackendSearcher.append_device)


def test_null_arguments_are_refused_without_a_device(la):
    L = la.lib()
    rows = np.zeros((4, 8), np.float32)
    p = rows.ctypes.data_as(la._native.f32p)
    for ld in (8, 6, 2, 0):                                    # a good pitch and three bad ones: the NULL handle is named either way
        out = C.c_void_p(0x1)
        assert L.leann_backend_append_device(None, rows.ctypes.data, 4, ld, C.byref(out)) == INVALID
        assert "null" in L.leann_last_error().decode() and not out.value
    out = C.c_void_p(0x1)
    assert L.leann_backend_append(None, p, 4, C.byref(out)) == INVALID and not out.value
    assert "leann_backend_append" in L.leann_last_error().decode()
    assert L.leann_backend_append(None, p, 4, None) == INVALID
    assert L.leann_backend_append_device(None, None, 0, 8, None) == INVALID
