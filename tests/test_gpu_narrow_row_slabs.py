"""-m gpu: the slab boundaries of the narrow row store (csrc/narrow_rows.hip), for bf16 and int8 rows alike.

The store moves rows in slabs: 64 MiB of store rows between the host and the store (an index file's rows going up, the export and
the save coming down), 256 MiB of f32 rows through the transient staging slab of host f32 rows.  Every other test index fits in one
slab; the cases here are the smallest that reach a second one, plus the empty and the single-row handle.

    store transfers   d = 8: a store row is 128 B for both types, one slab is 524 288 rows, n = 524 288 + 5
    f32 staging       d = 4096 (the widest row): one slab is 16 384 rows, n = 16 384 + 5

The handles are made with from_arrays over a hand-made DiskANN graph — a ring, adj0[i] = [(i + 1) % n], degree 1, no upper lists — so
neither a builder nor an oracle graph is on the path.  Every comparison is bit for bit against the host definitions: la.round_bf16
for bf16 rows, tests/i8_ref.py for int8 rows."""
import numpy as np
import pytest

import i8_ref

pytestmark = pytest.mark.gpu
STORE_SLAB_ROWS = (64 << 20) // 128      # d = 8
STAGE_SLAB_ROWS = (256 << 20) // (4096 * 4)  # d = 4096
ROW_TYPES = ["BF16", "I8"]


def _ring(la, X, row_type, entry=0):
    n = len(X)
    adj0 = ((np.arange(n, dtype=np.uint32) + 1) % max(n, 1)).astype(np.uint32).reshape(n, 1)
    return la.BackendSearcher.from_arrays(la.BackendType.DiskAnn, X, 1, 1, 0, entry, np.zeros(n, np.uint8), np.zeros(n, np.uint32), adj0,
                                          np.zeros((0, 1), np.uint32), row_type=row_type)


def _stored(la, s):
    """what the handle stores, as the raw export gives it: (bf16 bits,) or (exponents, codes)"""
    return (s.export_rows_bf16(),) if s.row_type() == la.RowType.BF16 else s.rows_export_i8()


def _defined(la, X, row_type):
    """the same from the host definition"""
    return (la.round_bf16(X),) if row_type == la.RowType.BF16 else i8_ref.quantize(X)


def _widened(la, stored, row_type):
    """the f32 rows the index is defined over: b << 16, or code x 2^-e"""
    if row_type == la.RowType.BF16:
        return (stored[0].astype(np.uint32) << 16).view(np.float32)
    return i8_ref.dequantize(stored[1], stored[0])


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and (x == y).all() for x, y in zip(a, b))


@pytest.fixture(scope="module")
def rows_d8():
    n = STORE_SLAB_ROWS + 5
    X = np.random.default_rng(0x51AB0008).standard_normal((n, 8)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    X.setflags(write=False)
    return X


@pytest.fixture(scope="module")
def rows_d4096():
    n = STAGE_SLAB_ROWS + 5
    X = np.random.default_rng(0x51AB1000).standard_normal((n, 4096)).astype(np.float32)
    X[STAGE_SLAB_ROWS + 2, 7] = 300.0   # column 7's exponent is decided in the second slab ...
    X[11, 9] = -500.0                   # ... and column 9's in the first
    X.setflags(write=False)
    return X


@pytest.mark.parametrize("rt", ROW_TYPES)
def test_store_transfers_cross_a_slab(la, gpu, rows_d8, rt, tmp_path):
    row_type, X, n = la.RowType[rt], rows_d8, len(rows_d8)
    target = STORE_SLAB_ROWS + 2  # row 524 290
    want = _defined(la, X, row_type)
    s = _ring(la, X, row_type, entry=STORE_SLAB_ROWS)
    try:
        assert s.row_type() == row_type and s.len() == n
        got = _stored(la, s)  # the download, slab by slab
        assert _same(got, want)
        for r in (STORE_SLAB_ROWS - 1, STORE_SLAB_ROWS):  # the last row of the first slab, the first of the second
            assert (got[-1][r] == want[-1][r]).all()
        Xw = _widened(la, want, row_type)
        V = s.graph_export(with_vectors=True)["vectors"]  # the in-place widening at full length
        assert (V.view(np.uint32) == Xw.view(np.uint32)).all()
        stem = str(tmp_path / "ring.leann")
        s.save(stem)
        s2 = la.DiskAnnSearcher.load(stem, 8)  # the upload of an index file's rows, slab by slab
        try:
            assert s2.row_type() == row_type and s2.len() == n
            assert _same(_stored(la, s2), want)
        finally:
            s2.close()
        keys, _ = s.search(Xw[target], 1, 32)  # the ring is walked from row 524 288 on
        assert keys.tolist() == [target]
    finally:
        s.close()


@pytest.mark.parametrize("rt", ROW_TYPES)
def test_f32_staging_crosses_a_slab(la, gpu, rows_d4096, rt):
    row_type, X = la.RowType[rt], rows_d4096
    assert np.abs(X[:, 7]).argmax() == STAGE_SLAB_ROWS + 2 and np.abs(X[:, 9]).argmax() == 11
    want = _defined(la, X, row_type)
    s = _ring(la, X, row_type)
    try:
        assert s.row_type() == row_type
        got = _stored(la, s)
        assert _same(got, want)  # int8: the column pass accumulated over both slabs, and the second upload
        for r in (STAGE_SLAB_ROWS - 1, STAGE_SLAB_ROWS):
            assert (got[-1][r] == want[-1][r]).all()
    finally:
        s.close()


@pytest.mark.parametrize("n", [0, 1])
@pytest.mark.parametrize("rt", ROW_TYPES)
def test_empty_and_single_row(la, gpu, rt, n, tmp_path):
    row_type, d = la.RowType[rt], 8
    X = np.random.default_rng(0x51AB0001).standard_normal((n, d)).astype(np.float32)
    want = _defined(la, X, row_type)
    s = _ring(la, X, row_type)
    try:
        assert s.row_type() == row_type and s.len() == n and s.dims() == d
        assert _same(_stored(la, s), want)
        V = s.graph_export(with_vectors=True)["vectors"]
        assert (V.view(np.uint32) == _widened(la, want, row_type).view(np.uint32)).all()
        stem = str(tmp_path / "tiny.leann")
        s.save(stem)
        s2 = la.DiskAnnSearcher.load(stem, d)
        try:
            assert s2.row_type() == row_type and s2.len() == n and s2.dims() == d
            assert _same(_stored(la, s2), want)
        finally:
            s2.close()
    finally:
        s.close()
