"""CPU suite: MXFP4 rows (csrc/scan_mx4.hip): leann_pack_mx4 and leann_quantize_query_mx8 against tests/mx4_rows_ref.py byte for byte,
the rounding of both against a nearest-value search over the 8 and 127 code values, and the new symbols of the ABI."""
import numpy as np
import pytest

import mx4_rows_ref as ref

DIMS = [1, 31, 32, 33, 255, 256, 257, 768, 4096]
NAMES = ["leann_mx4_rows_from_device", "leann_mx4_rows_from_host", "leann_mx4_rows_len", "leann_mx4_rows_dims", "leann_mx4_rows_code_pitch",
         "leann_mx4_rows_scale_pitch", "leann_mx4_rows_export", "leann_mx4_rows_close", "leann_pack_mx4", "leann_quantize_query_mx8",
         "leann_mx4_rows_search_batch_device", "leann_mx4_rows_search_batch", "leann_mx4_rows_search_refined_batch_device",
         "leann_mx4_rows_search_refined_batch"]


def _around(values):
    v = np.asarray(values, np.float32)
    return np.stack([v, np.nextafter(v, np.float32(0)), np.nextafter(v, np.float32(np.inf))], axis=1).reshape(-1)


def rows(dims, n=37):
    """normal rows of mixed magnitude per block, and in the leading block of the first rows every edge of the definition"""
    rng = np.random.default_rng(dims)
    X = (rng.standard_normal((n, dims)) * 2.0 ** rng.integers(-12, 12, (n, 1))).astype(np.float32)
    sign = np.where(np.arange(32) % 3 == 0, -1, 1).astype(np.float32)
    ties4 = np.resize(np.concatenate([[6.0], _around([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5])]), 32) * sign  # amax 6: y = x
    ties8 = np.concatenate([[500.0], _around([17, 19, 21, 23, 2.0 ** -10, 3 * 2.0 ** -10, 5 * 2.0 ** -10, 464]), [448, 449, 470, 479, 2.0 ** -9, 0, -0.0]]) * sign
    edge = [ties4, ties4 * 2.0 ** -40, ties8, ties8 / 64,                    # the two tables: y = x, and y = q for a query
            [7.5, -5.5, 6.5, 7.99, 5.0, 6.0], [450.0, -470, 511.9, 448, 449],  # block maxima in (6, 8) and in (448, 512): saturation
            [-0.0, np.nan, np.inf, -np.inf, 3.0, -0.4, 1e-3], np.zeros(32),   # what is not finite counts as 0; an all-zero block
            np.arange(32) * 1e-45, ties4 * 2.0 ** -131,                       # a denormal block
            ties4 * 2.0 ** -127, ties4 * 2.0 ** -126, ties4 * 2.0 ** 125]     # amax 1.5 x 2^-125, x 2^-124, x 2^127: E = 2, 3, 254
    edge.append(np.array(edge[-3]) / 2)                                       # E = 1
    for i, e in enumerate(edge):
        m = min(dims, 32, len(e))
        X[i, :min(dims, 32)] = 0
        X[i, :m] = np.asarray(e, np.float32)[:m]
    return X


def _nearest(y, values):
    """the code of the value nearest |y|, ties to the even code, saturating: what 'round to nearest even' means, by search"""
    d = np.abs(np.abs(y)[..., None] - values)
    best = d.argmin(axis=-1)
    tie = (np.take_along_axis(d, np.minimum(best + 1, len(values) - 1)[..., None], -1)[..., 0] == d.min(axis=-1)) & (best + 1 < len(values))
    return np.where(tie & (best % 2 == 1), best + 1, best)


@pytest.mark.parametrize("dims", DIMS)
def test_pack_equals_the_restatement(la, dims):
    X = rows(dims)
    codes, scales = la.pack_mx4(X)
    want = ref.pack(X)
    assert codes.shape == (37, 128 * ref.ktiles(dims)) and scales.shape == (37, 8 * ref.ktiles(dims))
    assert (codes == want[0]).all() and (scales == want[1]).all() and scales.max() < 255
    # the restatement's table is round-to-nearest-even over the eight E2M1 values
    P, A, E = ref._blocks(X)
    y = A.astype(np.float64) * 2.0 ** (127 - np.maximum(E - 2, 0))[:, :, None]
    nib = np.stack([codes & 15, codes >> 4], axis=2).reshape(y.shape)
    assert ((nib & 7) == _nearest(y, ref.E2M1))[np.isfinite(P)].all()
    assert (y.max(axis=2)[E >= 2] >= 4).all() and (y < 8).all()


@pytest.mark.parametrize("dims", DIMS)
def test_query_codes_equal_the_restatement(la, dims):
    values = ref.fp8_value(np.arange(127))  # 0 .. 448, ascending
    for q in rows(dims):
        codes, scales, finite = la.quantize_query_mx8(q)
        wc, ws, wf = ref.quantize_query(q)
        assert finite == wf == bool(np.isfinite(q).all())
        if not finite:
            assert (codes == 0).all() and (scales == 255).all()
            continue
        assert (codes == wc).all() and (scales == ws).all()
        P, A, E = ref._blocks(q)
        y = (A.astype(np.float64) * 2.0 ** (127 - np.maximum(E - 8, 0))[:, :, None]).reshape(-1)
        assert ((codes & 127) == _nearest(y, values)).all() and ((codes >> 7) == np.signbit(P).reshape(-1)).all()


def test_symbols_and_refusals(la):
    L = la.lib()
    assert all(hasattr(L, name) and name in la._native.SIGNATURES for name in NAMES)
    for call in (la.pack_mx4, lambda x: la.quantize_query_mx8(x[0])):
        with pytest.raises(la.LeannError) as e:
            call(np.zeros((2, 4097), np.float32))
        assert e.value.code == 1 and "dims" in str(e.value)
