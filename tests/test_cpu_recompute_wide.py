"""CPU suite: recompute search for dims above 768.  (1) The column-block plan of the general encode kernel
(leann-rs_amd/csrc/encode_plan.h) — host/encode_plan_selftest.cpp is built with the host compiler under AddressSanitizer + UBSan and
checks, for every dims in 1..4096 and h in {64, 100, 128, 256, 512, 1024}: dp >= dims and dp % 128 == 0; the blocks tile [0, dp)
exactly; every block width is a compiled tile count; dims <= 768 keeps the one-block plan (5 tiles -> 6); the LDS figure is
encode_lds_bytes of the widest block and <= 160 KiB whenever the plan is accepted.  (2) The argument checks of
leann_recompute_create, which come before any device work.  No GPU."""
import ctypes as C
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "leann-rs_amd", "host")
LEANN_ERR_INVALID, LEANN_ERR_DEVICE = 1, 4


def test_column_block_plan_for_every_width():
    exe = os.path.join(HOST, "encode_plan_selftest")
    subprocess.check_call(["make", "-s", "-C", ROOT, "leann-rs_amd/host/encode_plan_selftest"])  # a no-op when up to date
    p = subprocess.run([exe], stdout=subprocess.PIPE, check=False)
    r = json.loads(p.stdout)
    assert r["cases"] == 6 * 4096
    assert r["accepted"] == 4 * 4096  # h = 512 and 1024: the feature tile alone leaves no room for a slab ring, as before
    for key in ("bad_dp", "bad_tiling", "bad_width", "bad_narrow", "bad_lds", "bad_padding", "bad_limit"):
        assert r[key] == 0, r
    assert p.returncode == 0


def _create(la, dims, device):
    """leann_recompute_create with pointers that are never dereferenced: the calls below fail at the argument or device check."""
    L = la.lib()
    dummy = (C.c_uint16 * 8)()
    out = C.c_void_p()
    rc = L.leann_recompute_create(C.cast(dummy, C.c_void_p), 8, 256, C.cast(dummy, C.c_void_p), dims, device, 0, C.byref(out))
    return rc, L.leann_last_error().decode("utf-8", "replace"), out


def test_dims_limit_is_4096(la):
    # a device index no machine has: the device check (which follows the argument check) refuses it before any device work
    rc, msg, out = _create(la, 4097, 9999)
    assert rc == LEANN_ERR_INVALID and "4096" in msg and not out.value
    rc, msg, out = _create(la, 1536, 9999)
    assert rc == LEANN_ERR_DEVICE and "not available" in msg and not out.value  # LEANN_ERR_INVALID ("dims <= 768") before
    rc, msg, out = _create(la, 4096, 9999)
    assert rc == LEANN_ERR_DEVICE
    rc, msg, out = _create(la, 768, 9999)
    assert rc == LEANN_ERR_DEVICE
    rc, msg, out = _create(la, 0, 9999)
    assert rc == LEANN_ERR_INVALID


def test_host_twin_rejects_wide_dims_before_any_device_work(la):
    """leann_recompute_create_host uploads its inputs before it calls leann_recompute_create: its own argument check names the limit"""
    import numpy as np
    L = la.lib()
    u16p = C.POINTER(C.c_uint16)
    F, W = np.zeros((4, 16), np.uint16), np.zeros((16, 8), np.uint16)  # never read: dims = 4097 is refused first
    out = C.c_void_p()
    rc = L.leann_recompute_create_host(F.ctypes.data_as(u16p), 4, 16, W.ctypes.data_as(u16p), 4097, 9999, 0, C.byref(out))
    assert rc == LEANN_ERR_INVALID and b"4096" in L.leann_last_error() and not out.value
    rc = L.leann_recompute_create_host(F.ctypes.data_as(u16p), 4, 16, W.ctypes.data_as(u16p), 8, 9999, 0, C.byref(out))
    assert rc == LEANN_ERR_DEVICE and not out.value
