"""CPU suite: the flat search on int8 rows (include/leann_backend.h "exhaustive search on int8 rows") — leann_quantize_query_i8 against
tests/flat_i8_ref.py, and the refusals that come before a handle is read (those that need a handle: tests/test_gpu_flat_i8.py)."""
import ctypes as C

import numpy as np
import pytest

import flat_i8_ref

INVALID = 1
ULP_UP = lambda x: np.nextafter(np.float32(x), np.float32(np.inf))


def _cases():
    rng, d = np.random.default_rng(5), 40
    base, z = rng.standard_normal(d).astype(np.float32), np.zeros(d, np.int8)
    yield "random, mixed exponents", base, rng.integers(-9, 9, d).astype(np.int8)
    for name, amax in (("amax = 127 * 2^-7: m = 127/128, E = 7", 127 / 128), ("one ulp above: E = 6", ULP_UP(127 / 128)),
                       ("amax = 127 * 2^-E exactly, E = 3", 127 / 8), ("one ulp above 127 * 2^-3", ULP_UP(127 / 8)),
                       ("far below unit scale: E = 66 is not clamped", 2.0 ** -60), ("far above: E = -34", 1.5 * 2.0 ** 40)):
        q = (base / np.abs(base).max() * np.float32(0.7)).astype(np.float32) * np.float32(amax)
        q[7] = -np.float32(amax)
        yield name, q, z
    yield "all zero", np.zeros(d, np.float32), z
    e32 = z.copy()
    e32[::2], e32[1::2] = 32, -32
    yield "column exponents +-32", base, e32
    yield "a tie: 2.5 -> 2, 3.5 -> 4", np.array([127, 2.5, 3.5, -2.5, -126.5], np.float32), np.zeros(5, np.int8)
    for bad in (np.nan, np.inf, -np.inf):
        q = base.copy()
        q[11] = bad
        yield f"element {bad}", q, z
    yield "the scaled product overflows", np.full(d, 3e38, np.float32), np.full(d, -32, np.int8)


@pytest.mark.parametrize("name,q,e", list(_cases()), ids=[c[0] for c in _cases()])
def test_quantize_query_equals_the_restatement(la, name, q, e):
    codes, E = la.quantize_query_i8(q, e)
    rc, rE = flat_i8_ref.query_codes(q, e)
    assert E == rE and (codes == rc).all(), name
    if "E = " in name:
        assert E == int(name.split("E = ")[1].split()[0].rstrip(":,")), name
    if "element" in name or "overflows" in name:
        assert E == flat_i8_ref.NONFINITE == -2 ** 31 and not codes.any()


def test_entry_points_refuse_bad_arguments_before_the_handle_is_read(la):
    L = la.lib()
    blocks, err = L.leann_debug_device_blocks(), lambda: L.leann_last_error().decode()
    fake = C.c_void_p(0x1000)  # never dereferenced: every call below is refused first
    q = np.zeros(8, np.float32)
    keys, dists, cnt = np.zeros(4, np.uint64), np.zeros(4, np.float32), np.zeros(1, np.uint32)
    f32p, u64p, u32p, i8p = (C.POINTER(t) for t in (C.c_float, C.c_uint64, C.c_uint32, C.c_int8))
    dev = lambda **kw: L.leann_backend_search_flat_batch_device(*{**dict(h=fake, q=fake, nq=1, k=2, f=4, a=None, keys=fake, dists=fake,
                                                                         counts=fake, st=None), **kw}.values())
    host = lambda **kw: L.leann_backend_search_flat_batch(*{**dict(h=fake, q=q.ctypes.data_as(f32p), nq=1, k=2, f=4, a=None,
                                                                   keys=keys.ctypes.data_as(u64p), dists=dists.ctypes.data_as(f32p),
                                                                   counts=cnt.ctypes.data_as(u32p)), **kw}.values())
    for call, who in ((dev, "leann_backend_search_flat_batch_device"), (host, "leann_backend_search_flat_batch")):
        for arg, name in (("h", "handle"), ("q", "queries"), ("keys", "keys"), ("dists", "dists"), ("counts", "counts")):
            assert call(**{arg: None}) == INVALID and err() == f"{who}: null {name}"
        assert call(k=0) == INVALID and "top_k = 0" in err()
        assert call(k=5) == INVALID and "top_k = 5" in err() and "fetch_k = 4" in err()
        assert call(k=5, f=1025) == INVALID and "fetch_k = 1025" in err()
    e, c, E = np.zeros(8, np.int8), np.zeros(8, np.int8), C.c_int32(0)
    args = [q.ctypes.data_as(f32p), 8, e.ctypes.data_as(i8p), c.ctypes.data_as(i8p), C.byref(E)]
    for i, name in ((0, "q"), (2, "exps"), (3, "codes_out"), (4, "E_out")):
        assert L.leann_quantize_query_i8(*[None if j == i else a for j, a in enumerate(args)]) == INVALID and f"null {name}" in err()
    assert L.leann_quantize_query_i8(*[0 if j == 1 else a for j, a in enumerate(args)]) == INVALID and "d = 0" in err()
    assert L.leann_debug_device_blocks() == blocks  # refused calls own nothing
