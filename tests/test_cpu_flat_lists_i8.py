"""CPU suite: the int8 flat search over per-query lists and bitmaps (include/leann_backend.h "exhaustive search on int8 rows, per
query") — the refusals that come before a handle is read (those that need a handle: tests/test_gpu_flat_lists_i8.py)."""
import ctypes as C

import numpy as np

INVALID = 1


def test_entry_points_refuse_bad_arguments_before_the_handle_is_read(la):
    L = la.lib()
    blocks, err = L.leann_debug_device_blocks(), lambda: L.leann_last_error().decode()
    fake = C.c_void_p(0x1000)  # never dereferenced: every call below is refused first
    q, allow = np.zeros(16, np.float32), np.zeros(64, np.uint8)
    keys, dists, cnt = np.zeros(8, np.uint64), np.zeros(8, np.float32), np.zeros(2, np.uint32)
    f32p, u64p, u32p, u8p = (C.POINTER(t) for t in (C.c_float, C.c_uint64, C.c_uint32, C.c_uint8))
    host_out = dict(keys=keys.ctypes.data_as(u64p), dists=dists.ctypes.data_as(f32p), counts=cnt.ctypes.data_as(u32p))
    off = lambda *v: np.array(v, np.uint64).ctypes.data_as(u64p)
    ql = lambda *v: np.array(v, np.uint32).ctypes.data_as(u32p)
    lists_dev = lambda **kw: L.leann_backend_search_flat_lists_batch_device(*{**dict(
        h=fake, q=fake, nq=2, k=2, f=4, off=off(0, 3, 5), lists=fake, nl=2, ql=None, keys=fake, dists=fake, counts=fake, sk=None, st=None), **kw}.values())
    lists_host = lambda **kw: L.leann_backend_search_flat_lists_batch(*{**dict(
        h=fake, q=q.ctypes.data_as(f32p), nq=2, k=2, f=4, off=off(0, 3, 5), lists=ql(1, 2, 3, 4, 5), nl=2, ql=None, **host_out, sk=None), **kw}.values())
    filt_dev = lambda **kw: L.leann_backend_search_flat_filtered_batch_device(*{**dict(
        h=fake, q=fake, nq=2, k=2, f=4, a=fake, stride=32, keys=fake, dists=fake, counts=fake, st=None), **kw}.values())
    filt_host = lambda **kw: L.leann_backend_search_flat_filtered_batch(*{**dict(
        h=fake, q=q.ctypes.data_as(f32p), nq=2, k=2, f=4, a=allow.ctypes.data_as(u8p), stride=32, **host_out), **kw}.values())
    for call, who in ((lists_dev, "leann_backend_search_flat_lists_batch_device"), (lists_host, "leann_backend_search_flat_lists_batch"),
                      (filt_dev, "leann_backend_search_flat_filtered_batch_device"), (filt_host, "leann_backend_search_flat_filtered_batch")):
        for arg, name in (("h", "handle"), ("q", "queries"), ("keys", "keys"), ("dists", "dists"), ("counts", "counts")):
            assert call(**{arg: None}) == INVALID and err() == f"{who}: null {name}"
        assert call(k=0) == INVALID and err() == f"{who}: top_k = 0"
        assert call(k=5) == INVALID and "top_k = 5" in err() and "fetch_k = 4" in err()
        assert call(k=5, f=1025) == INVALID and "fetch_k = 1025" in err()
        if "lists" not in who:
            continue
        assert call(off=None) == INVALID and err() == f"{who}: null list_off"
        assert call(lists=None) == INVALID and err() == f"{who}: null lists"
        assert call(off=off(1, 3, 5)) == INVALID and "list_off[0] = 1" in err()
        assert call(off=off(0, 5, 3)) == INVALID and "list_off[2] = 3 after 5" in err()
        assert call(off=off(0, 2 ** 31, 2 ** 31)) == INVALID and "shorter than 2^31" in err()
        assert call(nl=1) == INVALID and "q_list is null" in err() and "n_lists = 1" in err() and "nq = 2" in err()
        assert call(ql=ql(1, 2)) == INVALID and "q_list[1] = 2" in err() and err().startswith(who + ":")
    assert L.leann_debug_device_blocks() == blocks  # refused calls own nothing
