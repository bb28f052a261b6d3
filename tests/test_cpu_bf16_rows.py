"""CPU suite for the bf16 row type: the library's rounding (leann_round_bf16, csrc/bf16.h) against the numpy restatement of
tests/bf16_ref.py, bit for bit; version-3 index files are validated like versions 1 and 2 before anything reaches a device; the new
entry points refuse an unknown row type and null outputs without a device.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import bf16_ref
from util import synth

u16p = C.POINTER(C.c_uint16)


def _round(la, bits):
    x = np.ascontiguousarray(bits, np.uint32).view(np.float32)
    out = la.round_bf16(x)
    assert out.dtype == np.uint16 and out.shape == x.shape
    return out


def test_round_crafted_patterns(la):
    cases = {
        0x3F808000: 0x3F80,  # tie, even below: down
        0x3F818000: 0x3F82,  # tie, odd below: up
        0x3F807FFF: 0x3F80, 0x3F808001: 0x3F81,  # one ulp to either side of the first tie
        0x3F817FFF: 0x3F81, 0x3F818001: 0x3F82,  # ... and of the second
        0x00000000: 0x0000, 0x80000000: 0x8000,  # +-0
        0x00000001: 0x0000, 0x80000001: 0x8000, 0x00008000: 0x0000, 0x00008001: 0x0001, 0x00018000: 0x0002,  # denormals
        0x007FFFFF: 0x0080, 0x807FFFFF: 0x8080,  # the largest denormal rounds up to the smallest normal
        0x7F800000: 0x7F80, 0xFF800000: 0xFF80,  # +-inf
        0x7F7FFFFF: 0x7F80, 0xFF7FFFFF: 0xFF80,  # the largest finite value rounds to infinity
        0x7F7F7FFF: 0x7F7F,
    }
    bits = np.array(list(cases), np.uint32)
    want = np.array(list(cases.values()), np.uint16)
    got = _round(la, bits)
    assert (got == want).all(), [(hex(b), hex(g), hex(w)) for b, g, w in zip(bits, got, want) if g != w]
    assert (bf16_ref.round_bf16(bits.view(np.float32)) == want).all()


def test_round_nans_stay_nans(la):
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7FC12345, 0x7F800001, 0xFF800001, 0x7FA00000, 0xFFBFFFFF, 0x7F80FFFF, 0x7FFFFFFF, 0xFFFFFFFF],
                    np.uint32)  # quiet and signalling, both signs, payloads that live in the low half only
    got = _round(la, nans)
    assert ((got & 0x7F80) == 0x7F80).all() and ((got & 0x007F) != 0).all()  # still NaN
    assert ((got >> 15) == (nans >> 31)).all()                              # the sign is kept
    assert (got == bf16_ref.round_bf16(nans.view(np.float32))).all()
    assert np.isnan(bf16_ref.widen(got)).all()


def test_round_random_bit_patterns(la):
    bits = np.random.default_rng(0x5EED0001).integers(0, 2 ** 32, 100_000, dtype=np.uint64).astype(np.uint32)
    got, want = _round(la, bits), bf16_ref.round_bf16(bits.view(np.float32))
    assert (got == want).all(), int((got != want).sum())
    x = bits.view(np.float32)
    fin = np.isfinite(x) & np.isfinite(bf16_ref.widen(got))
    # round to nearest: the error is at most half a bf16 ulp of the result's binade (2^-8 relative, 2^-134 absolute for denormals)
    err = np.abs(bf16_ref.widen(got)[fin].astype(np.float64) - x[fin].astype(np.float64))
    assert (err <= np.maximum(np.abs(x[fin].astype(np.float64)) * 2.0 ** -8, 2.0 ** -134)).all()
    assert (bf16_ref.round_bf16(bf16_ref.widen(got)) == got).all()  # r(w(b)) = b: rounding is idempotent


def test_round_null_arguments(la):
    L = la.lib()
    out = np.zeros(4, np.uint16)
    assert L.leann_round_bf16(None, 4, out.ctypes.data_as(u16p)) == 1 and b"null" in L.leann_last_error()
    x = np.zeros(4, np.float32)
    assert L.leann_round_bf16(x.ctypes.data_as(C.POINTER(C.c_float)), 4, None) == 1
    assert L.leann_round_bf16(None, 0, None) == 0


# ---- version-3 index files ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def good(po):
    X = synth(po, 300, 32)
    G = po.Graph.build_hnsw(X, M=4, efc=16)
    lv, uo, a0, aU = G.export()
    return dict(rows_bf16=bf16_ref.round_bf16(X), M=4, M0=8, max_level=G.max_level, entry=G.entry, levels=lv, upper_off=uo, adj0=a0, adjU=aU)


def _open(la, tmp_path, kind=0, dims=32, device=0):
    return la.BackendSearcher.load(kind, str(tmp_path / "documents.leann"), dims, device)


def test_v3_well_formed_file_reaches_the_device(la, good, tmp_path):
    bf16_ref.write_gx3(tmp_path / "documents.index", 0, **good)
    n_graph = 300 + 4 * 300 + 4 * 300 * 8 + 4 * good["adjU"].size
    assert (tmp_path / "documents.index").stat().st_size == 128 + n_graph + 300 * 32 * 2
    if la.device_count() > 0:
        s = _open(la, tmp_path)
        assert s.len() == 300 and s.row_type() == la.RowType.BF16
        s.close()
    else:
        with pytest.raises(la.LeannError) as e:
            _open(la, tmp_path)
        assert e.value.code == 4 and "no CPU fallback" in str(e.value)  # validation passed; only the GPU is missing


def test_v3_truncated_and_padded_files(la, good, tmp_path):
    bf16_ref.write_gx3(tmp_path / "documents.index", 0, **good)
    raw = (tmp_path / "documents.index").read_bytes()
    for cut in (len(raw) - 1, len(raw) - 300 * 32, len(raw) - 300 * 32 * 2, len(raw) // 2, 128):  # truncated rows, no rows, less
        (tmp_path / "documents.index").write_bytes(raw[:cut])
        with pytest.raises(la.LeannError) as e:
            _open(la, tmp_path)
        assert e.value.code == 3, cut
    (tmp_path / "documents.index").write_bytes(raw + b"\0")  # one byte too long
    with pytest.raises(la.LeannError, match="file length does not match the header") as e:
        _open(la, tmp_path)
    assert e.value.code == 3
    # the same payload under version 1 is half an f32 payload: the version decides how the rows are counted
    b = bytearray(raw)
    b[8:12] = (1).to_bytes(4, "little")
    (tmp_path / "documents.index").write_bytes(bytes(b))
    with pytest.raises(la.LeannError, match="file length does not match the header"):
        _open(la, tmp_path)


def test_v3_graph_arrays_are_validated(la, good, tmp_path):
    g = dict(good)
    a0 = good["adj0"].copy(); a0[17, 3] = 300  # neighbour id >= n: an out-of-bounds row read in the traversal kernel
    g["adj0"] = a0
    bf16_ref.write_gx3(tmp_path / "documents.index", 0, **g)
    with pytest.raises(la.LeannError) as e:
        _open(la, tmp_path)
    assert e.value.code == 3 and "level-0 neighbour id >= n" in str(e.value)
    top = int(np.argmax(good["levels"]))
    g = dict(good)
    aU = good["adjU"].copy(); aU[good["upper_off"][top], 0] = 305
    g["adjU"] = aU
    bf16_ref.write_gx3(tmp_path / "documents.index", 0, **g)
    with pytest.raises(la.LeannError) as e:
        _open(la, tmp_path)
    assert e.value.code == 3 and "upper-level neighbour id >= n" in str(e.value)


def test_v3_sharded_open_is_refused_without_a_device(la, good, tmp_path):
    bf16_ref.write_gx3(tmp_path / "documents.index", 0, **good)
    with pytest.raises(la.LeannError) as e:
        _open(la, tmp_path, device="0,0")
    assert e.value.code == 5 and "leann_sharded_from_handles" in str(e.value)


# ---- argument checks of the new entry points ----------------------------------------------------------------------------------------
def test_new_entry_points_reject_bad_arguments_without_a_gpu(la, good, tmp_path):
    L = la.lib()
    X = bf16_ref.widen(good["rows_bf16"])
    f32p, u8p, u32p = (C.POINTER(t) for t in (C.c_float, C.c_uint8, C.c_uint32))
    lv, uo, a0, aU = (np.ascontiguousarray(good[k]) for k in ("levels", "upper_off", "adj0", "adjU"))
    nul = aU.size // 4

    def from_arrays(row_type, out):
        return L.leann_backend_from_arrays_rows(0, X.ctypes.data_as(f32p), 300, 32, 4, 8, good["max_level"], good["entry"], lv.ctypes.data_as(u8p),
                                                uo.ctypes.data_as(u32p), a0.ctypes.data_as(u32p), aU.ctypes.data_as(u32p), nul, 0, 0, row_type, out)

    h = C.c_void_p()
    for bad in (2, 3, -1, 77):  # LEANN_ROWS_FEATURES names a handle's type; it cannot be asked for
        assert from_arrays(bad, C.byref(h)) == 1 and b"row type" in L.leann_last_error() and not h.value, bad
        assert L.leann_backend_build_device_rows(0, None, 0, 32, 32, 4, 16, 0, 0, bad, 0, C.byref(h)) == 1 and b"row type" in L.leann_last_error()
        assert L.leann_backend_build_rows(0, X.ctypes.data_as(f32p), 300, 32, 4, 16, bad, str(tmp_path / "x.leann").encode()) == 1
        assert b"row type" in L.leann_last_error()
    assert not (tmp_path / "x.index").exists()
    assert from_arrays(1, None) == 1 and b"null" in L.leann_last_error()
    assert L.leann_backend_build_device_rows(0, None, 0, 32, 32, 4, 16, 0, 0, 1, 0, None) == 1 and b"null" in L.leann_last_error()
    assert L.leann_backend_to_rows(None, 1, C.byref(h)) == 1 and b"null" in L.leann_last_error()
    assert L.leann_backend_rows_export_bf16(None, None) == 1 and b"null" in L.leann_last_error()
    assert L.leann_backend_build_rows(0, X.ctypes.data_as(f32p), 300, 32, 4, 16, 1, None) == 1
    assert L.leann_backend_build_rows(0, X.ctypes.data_as(f32p), 300, 32, 1000, 16, 1, str(tmp_path / "x.leann").encode()) == 1  # degree
    assert L.leann_backend_row_type(None) == -1
    if la.device_count() == 0:  # well-formed requests stop at the device check: nothing computes on the CPU
        assert from_arrays(1, C.byref(h)) == 4 and b"no CPU fallback" in L.leann_last_error()
        assert L.leann_backend_build_rows(0, X.ctypes.data_as(f32p), 300, 32, 4, 16, 1, str(tmp_path / "x.leann").encode()) == 4
    # an inconsistent graph is refused before the device, whatever the row type
    bad0 = a0.copy(); bad0[1, 1] = 300
    rc = L.leann_backend_from_arrays_rows(0, X.ctypes.data_as(f32p), 300, 32, 4, 8, good["max_level"], good["entry"], lv.ctypes.data_as(u8p),
                                          uo.ctypes.data_as(u32p), bad0.ctypes.data_as(u32p), aU.ctypes.data_as(u32p), nul, 0, 0, 1, C.byref(h))
    assert rc == 3
