"""CPU suite for the int8 row type (include/leann_backend.h "row types", csrc/i8_rows.h): the library's reference quantiser
(leann_quantize_i8) against the numpy restatement of tests/i8_ref.py, bit for bit; version-4 index files are validated like every
other version before anything reaches a device; the int8 row type (4) passes the argument checks that 3 and 7 fail; and the plans of
the I8 family (csrc/search_plan.h through host/search_plan_selftest) against expectations written by hand.  No GPU needed."""
import ctypes as C
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import i8_ref
from util import synth

i8p = C.POINTER(C.c_int8)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELFTEST = os.path.join(ROOT, "leann-rs_amd", "host", "search_plan_selftest")
INVALID, FORMAT, DEVICE, UNSUPPORTED = 1, 3, 4, 5


def _same_as_ref(la, X):
    e, c = la.quantize_i8(X)
    re, rc = i8_ref.quantize(X)
    assert e.dtype == np.int8 and c.dtype == np.int8 and e.shape == (X.shape[1],) and c.shape == X.shape
    assert (e == re).all(), [(j, int(e[j]), int(re[j])) for j in np.flatnonzero(e != re)[:8]]
    assert (c == rc).all(), int((c != rc).sum())
    assert (c != -128).all() and (np.abs(e.astype(int)) <= 32).all()
    return e, c


# ---- the quantiser ------------------------------------------------------------------------------------------------------------------
def test_quantize_seeded_rows(la, po):
    for n, d in ((300, 32), (257, 131), (64, 768)):
        X = synth(po, n, d)
        e, c = _same_as_ref(la, X)
        assert (np.abs(c.astype(int)).max(axis=0) >= 64).all()  # e_j is the LARGEST exponent that fits: every column uses its top bit
        Xq = i8_ref.dequantize(c, e)
        assert (np.abs(Xq.astype(np.float64) - X) <= np.ldexp(0.5, -e.astype(int))[None, :]).all()  # half a step of the column
    X = np.random.default_rng(3).standard_normal((500, 40)).astype(np.float32) * np.ldexp(1.0, np.arange(40) - 20).astype(np.float32)
    e, _ = _same_as_ref(la, X)
    assert len(set(e.tolist())) > 20  # one exponent per column, not one per matrix


def test_quantize_crafted_columns(la):
    f = np.float32
    top = f(127 * 2.0 ** -5)  # amax exactly at 127 2^-e: e = 5 fits, the codes reach 127
    X = np.zeros((8, 8), f)
    X[:, 0] = [0.3, -0.7, 0.11, 0.9, -0.95, 0.5, 0.25, -0.125]
    X[:, 1] = 0                                                  # a zero column: e = 0, codes 0
    X[:, 2] = [top, -top, 0.5 / 32, 1.5 / 32, 2.5 / 32, -0.5 / 32, -1.5 / 32, -2.5 / 32]  # ties at .5 go to the even code
    X[:, 3] = [np.nextafter(top, f(np.inf)), 0.5 / 16, 1.5 / 16, -3.5 / 16, 0, 0, 0, 0]  # one ulp above: e drops to 4
    X[:, 4] = [2.0 ** -40, -(2.0 ** -40), 2.0 ** -41, 0, 2.0 ** -60, 0, 0, 0]             # e clamps at +32
    X[:, 5] = [2.0 ** 50, -(2.0 ** 50), 100 * 2.0 ** 32, -126.5 * 2.0 ** 32, 127.5 * 2.0 ** 32, 2.0 ** 31, -(2.0 ** 31), 3 * 2.0 ** 31]  # ... at -32
    X[:, 6] = [1e-45, -1e-45, 0, 0, 0, 0, 0, 1e-44]              # subnormal amax
    X[:, 7] = [127, -127, 126.5, 125.5, -126.5, 63.5, 0.5, -0.5]  # e = 0
    e, c = _same_as_ref(la, X)
    assert e.tolist() == [7, 0, 5, 4, 32, -32, 32, 0]
    assert c[:, 1].tolist() == [0] * 8
    assert c[:, 2].tolist() == [127, -127, 0, 2, 2, 0, -2, -2]
    assert c[:, 3].tolist() == [64, 0, 2, -4, 0, 0, 0, 0]  # 127 2^-5 (1 + 2^-23) 2^4 = 63.50000757 -> 64
    assert c[:, 4].tolist() == [0] * 8                      # 2^-40 2^32 = 2^-8 -> 0
    assert c[:, 5].tolist() == [127, -127, 100, -126, 127, 0, 0, 2]  # saturation to +-127, never -128; 0.5 -> 0, 1.5 -> 2
    assert c[:, 6].tolist() == [0] * 8
    assert c[:, 7].tolist() == [127, -127, 126, 126, -126, 64, 0, 0]


def test_quantize_refuses_non_finite_values(la):
    L = la.lib()
    for bad in (np.nan, np.inf, -np.inf):
        X = np.ones((5, 6), np.float32)
        X[3, 2] = bad
        X[4, 1] = bad  # the FIRST one in row-major order is named
        with pytest.raises(la.LeannError) as e:
            la.quantize_i8(X)
        assert e.value.code == INVALID and "row 3, column 2" in str(e.value)
    e = np.zeros(4, np.int8)
    assert L.leann_quantize_i8(None, 2, 4, e.ctypes.data_as(i8p), e.ctypes.data_as(i8p)) == INVALID and b"null" in L.leann_last_error()
    assert L.leann_quantize_i8(None, 0, 4, e.ctypes.data_as(i8p), None) == 0 and (e == 0).all()  # no rows: every column is a zero column


# ---- version-4 index files ----------------------------------------------------------------------------------------------------------
def write_gx4(path, kind, exps, codes, M, M0, max_level, entry, levels, upper_off, adj0, adjU, efc=64, alpha=1.2, version=4):
    """a version-4 LEANNGX1 index file (csrc/indexfile.hip): the header and graph arrays of version 1, then int8 exps [d] and the codes
    int8 [n x d] in element order"""
    B = np.ascontiguousarray(codes, np.int8)
    n, d = B.shape
    adjU = np.ascontiguousarray(adjU, np.uint32).reshape(-1, M) if np.size(adjU) else np.zeros((0, M), np.uint32)
    hd = struct.pack("<8sIIQIIIIIIfIQI60x", b"LEANNGX1", version, kind, n, d, M, M0, max_level, entry, efc, alpha, 0, adjU.shape[0], 0)
    assert len(hd) == 128
    with open(path, "wb") as f:
        f.write(hd)
        f.write(np.ascontiguousarray(levels, np.uint8).tobytes())
        f.write(np.ascontiguousarray(upper_off, np.uint32).tobytes())
        f.write(np.ascontiguousarray(adj0, np.uint32).tobytes())
        f.write(adjU.tobytes())
        f.write(np.ascontiguousarray(exps, np.int8).tobytes())
        f.write(B.tobytes())


@pytest.fixture(scope="module")
def good(po):
    X = synth(po, 300, 32)
    G = po.Graph.build_hnsw(X, M=4, efc=16)
    lv, uo, a0, aU = G.export()
    e, c = i8_ref.quantize(X)
    return dict(exps=e, codes=c, M=4, M0=8, max_level=G.max_level, entry=G.entry, levels=lv, upper_off=uo, adj0=a0, adjU=aU), X


def _open(la, tmp_path, device=0):
    return la.BackendSearcher.load(0, str(tmp_path / "documents.leann"), 32, device)


def _refused(la, tmp_path, needle):
    with pytest.raises(la.LeannError) as e:
        _open(la, tmp_path)
    assert e.value.code == FORMAT and needle in str(e.value), str(e.value)


def test_v4_well_formed_file_reaches_the_device(la, good, tmp_path):
    g, _ = good
    write_gx4(tmp_path / "documents.index", 0, **g)
    n_graph = 300 + 4 * 300 + 4 * 300 * 8 + 4 * g["adjU"].size
    assert (tmp_path / "documents.index").stat().st_size == 128 + n_graph + 32 + 300 * 32
    if la.device_count() > 0:
        s = _open(la, tmp_path)
        assert s.len() == 300 and s.row_type() == la.RowType.I8
        s.close()
    else:
        with pytest.raises(la.LeannError) as e:
            _open(la, tmp_path)
        assert e.value.code == DEVICE and "no CPU fallback" in str(e.value)  # validation passed; only the GPU is missing
    with pytest.raises(la.LeannError) as e:  # a device list: refused before any device is looked at
        _open(la, tmp_path, device="0,0")
    assert e.value.code == UNSUPPORTED and "int8" in str(e.value) and "leann_sharded_from_handles" in str(e.value)


def test_v4_malformed_files_are_refused(la, good, tmp_path):
    g, X = good
    path = tmp_path / "documents.index"
    write_gx4(path, 0, **g)
    raw = path.read_bytes()
    path.write_bytes(raw[:-1])  # truncated by one byte
    _refused(la, tmp_path, "file length does not match the header")
    path.write_bytes(raw + b"\0")
    _refused(la, tmp_path, "file length does not match the header")
    for bad in (33, -33):
        e = g["exps"].copy(); e[5] = bad
        write_gx4(path, 0, **dict(g, exps=e))
        _refused(la, tmp_path, "exponent")
    c = g["codes"].copy(); c[299, 31] = -128
    write_gx4(path, 0, **dict(g, codes=c))
    _refused(la, tmp_path, "-128")
    # a version-1 payload (f32 rows, no exponents) under version 4: the version decides how the rows are counted
    v1 = raw[: len(raw) - 32 - 300 * 32] + np.ascontiguousarray(X, np.float32).tobytes()
    path.write_bytes(v1)
    _refused(la, tmp_path, "file length does not match the header")
    # ... and the graph arrays are validated as in every other version
    a0 = g["adj0"].copy(); a0[17, 3] = 300
    write_gx4(path, 0, **dict(g, adj0=a0))
    _refused(la, tmp_path, "level-0 neighbour id >= n")
    b = bytearray(raw); b[8:12] = (7).to_bytes(4, "little")
    path.write_bytes(bytes(b))
    _refused(la, tmp_path, "unsupported version")


# ---- argument checks ----------------------------------------------------------------------------------------------------------------
def test_the_int8_row_type_passes_argument_validation_where_3_and_7_do_not(la, good, tmp_path):
    L = la.lib()
    g, X = good
    f32p, u8p, u32p = (C.POINTER(t) for t in (C.c_float, C.c_uint8, C.c_uint32))
    lv, uo, a0, aU = (np.ascontiguousarray(g[k]) for k in ("levels", "upper_off", "adj0", "adjU"))

    def from_arrays(row_type, out):
        return L.leann_backend_from_arrays_rows(0, X.ctypes.data_as(f32p), 300, 32, 4, 8, g["max_level"], g["entry"], lv.ctypes.data_as(u8p),
                                                uo.ctypes.data_as(u32p), a0.ctypes.data_as(u32p), aU.ctypes.data_as(u32p), aU.size // 4, 0, 0, row_type, out)

    assert L.leann_backend_row_type(None) == -1
    h = C.c_void_p()
    I8 = int(la.RowType.I8)
    assert I8 == 4
    for bad in (3, 7):  # 3 was refused before there were int8 rows and stays unassigned
        assert from_arrays(bad, C.byref(h)) == INVALID and b"row type" in L.leann_last_error() and not h.value
        assert L.leann_backend_build_rows(0, X.ctypes.data_as(f32p), 300, 32, 4, 16, bad, str(tmp_path / "x.leann").encode()) == INVALID
    assert L.leann_backend_to_rows(None, I8, C.byref(h)) == INVALID and b"null" in L.leann_last_error()
    assert L.leann_backend_rows_export_i8(None, None, None) == INVALID and b"null" in L.leann_last_error()
    assert from_arrays(I8, None) == INVALID and b"null" in L.leann_last_error()
    rc = from_arrays(I8, C.byref(h))
    if la.device_count() == 0:  # a well-formed request stops at the device check: nothing computes on the CPU
        assert rc == DEVICE and b"no CPU fallback" in L.leann_last_error() and not h.value
        assert L.leann_backend_build_rows(0, X.ctypes.data_as(f32p), 300, 32, 4, 16, I8, str(tmp_path / "x.leann").encode()) == DEVICE
    else:
        assert rc == 0 and L.leann_backend_row_type(h) == I8
        L.leann_backend_close(h)
    assert not (tmp_path / "x.index").exists()


# ---- plans of the I8 family ---------------------------------------------------------------------------------------------------------
# d -> T, R of the 4-wave form, R of the 16-wave form (None: that width has none and small batches run 4 waves), visited-table bits at ef 64
PLAN_WIDTHS = {128: (1, 16, 4, 12), 260: (2, 12, 4, 12), 768: (3, 12, 4, 13), 1024: (4, 12, 4, 13), 1100: (6, 8, 4, 13), 1600: (8, 6, 3, 13),
               2820: (12, 4, 1, 13), 3400: (16, 4, None, 13)}
# LDS bytes at ef = 64, k = 10: (lists of <= 32 ids | of <= 80 ids) x (waves) x (plain, filtered), without the visited table —
# 2 x 64 x 8 + nbuf x ((deg + 8) x 8 + deg x 4) + 64, filtered + 2 x 10 x 8 + nbuf x (deg + 8) x 8; nbuf = 2 for 16 waves, 1 for 4
LDS = {(32, 16): (1984, 2784), (32, 4): (1536, 2016), (80, 16): (3136, 4704), (80, 4): (2112, 2976)}


def _plans(lines):
    p = subprocess.run([SELFTEST, "--plans"], input="".join(" ".join(str(v) for v in row) + "\n" for row in lines).encode(),
                       stdout=subprocess.PIPE, check=True)
    return [json.loads(x) for x in p.stdout.decode().splitlines()]


def test_i8_plans_match_hand_written_expectations():
    lines, want = [], []
    for d, (T, r4, r16, bits) in PLAN_WIDTHS.items():
        ld = (d + 3) & ~3
        for nq in (64, 704):
            nw = 16 if nq <= 512 and r16 is not None else 4
            r = r16 if nw == 16 else r4
            for filtered in (0, 1):
                for deg in (32, 80):
                    lines.append((ld, d, 0, 0, deg, 0, nq, 10, 64, filtered, 0, 0, 0, 0, 1))
                    name = f"{'wide_' if deg > 64 else ''}i8_beam_search{'_filtered' if filtered else ''}_kernel<{T}, {r}, {nw}>"
                    want.append(dict(err=0, msg="", family="I8", name=name, hash_bits=bits, lds_bytes=LDS[deg, nw][filtered] + 4 * 2 ** bits))
    got = _plans(lines)
    assert len(got) == len(want) == 8 * 2 * 2 * 2
    for line, g, w in zip(lines, got, want):
        assert g == w, (line, g, w)


def test_i8_plans_knobs_and_refusals():
    got = _plans([
        (768, 768, 0, 0, 32, 1, 704, 10, 64, 0, 0, 0, 16, 0, 1),   # LEANN_DEBUG_NW is ignored, and planes never matter
        (768, 768, 0, 0, 32, 0, 512, 10, 64, 0, 0, 0, 0, 0, 1),    # the BF16 batch threshold: 512 | 513
        (768, 768, 0, 0, 32, 0, 513, 10, 64, 0, 0, 0, 0, 0, 1),
        (768, 768, 0, 0, 32, 0, 64, 10, 64, 0, 0, 8, 0, 0, 1),     # LEANN_DEBUG_HASH_BITS wins
        (768, 768, 0, 0, 32, 0, 64, 10, 64, 0, 1, 0, 0, 0, 1),     # a construction search
        (4100, 4097, 0, 0, 32, 0, 64, 10, 64, 0, 0, 0, 0, 0, 1),
    ])
    assert [g["name"] for g in got[:4]] == ["i8_beam_search_kernel<3, 12, 4>", "i8_beam_search_kernel<3, 4, 16>", "i8_beam_search_kernel<3, 12, 4>",
                                            "i8_beam_search_kernel<3, 4, 16>"]
    assert got[3]["hash_bits"] == 8 and got[3]["lds_bytes"] == 1984 + 4 * 256
    assert got[4]["err"] == UNSUPPORTED and got[4]["msg"] == "int8 rows: construction searches are not supported"
    assert got[5]["err"] == INVALID and got[5]["msg"] == "search: dims 4097 > 4096 not supported"


def test_fourteen_column_lines_still_give_the_old_answers():
    got = _plans([
        (768, 768, 0, 0, 32, 0, 704, 10, 64, 0, 0, 0, 0, 0),
        (768, 768, 0, 1, 32, 0, 64, 10, 64, 1, 0, 0, 0, 0),
        (768, 768, 0, 1, 32, 0, 64, 10, 64, 0, 1, 0, 0, 0),
        (768, 768, 0, 0, 32, 0, 704, 10, 64, 0, 0, 0, 0, 0, 0),  # the extra column, off
    ])
    assert (got[0]["family"], got[0]["name"], got[0]["hash_bits"], got[0]["lds_bytes"]) == ("F32", "beam_search_kernel<3, 4, 4, false>", 13, 34304)
    assert (got[1]["family"], got[1]["name"], got[1]["lds_bytes"]) == ("BF16", "bf16_beam_search_filtered_kernel<3, 4, 16>", 35552)
    assert got[2]["err"] == UNSUPPORTED and got[2]["msg"] == "bf16 rows: construction searches are not supported"
    assert got[3] == got[0]
