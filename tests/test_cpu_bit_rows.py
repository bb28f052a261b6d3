"""CPU suite: sign-bit rows (include/leann_backend.h "sign-bit rows", csrc/scan_bits.hip) — what needs no GPU: the host pack reference
against numpy's packbits and against tests/bit_rows_ref.py, and the new symbols of the ABI."""
import numpy as np
import pytest

import bit_rows_ref

NAMES = ["leann_bit_rows_from_device", "leann_bit_rows_from_host", "leann_bit_rows_len", "leann_bit_rows_dims", "leann_bit_rows_pitch",
         "leann_bit_rows_export", "leann_bit_rows_close", "leann_pack_sign_bits", "leann_bit_rows_search_batch_device",
         "leann_bit_rows_search_batch", "leann_bit_rows_search_refined_batch_device", "leann_bit_rows_search_refined_batch"]


def rows(dims, n=37):
    """normal rows with the edge cases of the comparison sprinkled in: a NaN, +0, -0, and elements equal to the centre"""
    rng = np.random.default_rng(dims)
    X, c = rng.standard_normal((n, dims)).astype(np.float32), (0.3 * rng.standard_normal(dims)).astype(np.float32)
    X[1, 0], X[2, -1], X[3, dims // 2], X[4] = np.nan, 0.0, -0.0, c
    X[5, ::3] = 0.0
    X[6, ::2] = -0.0
    c[dims // 3] = np.nan if dims > 8 else c[dims // 3]
    return X, c


@pytest.mark.parametrize("centred", [False, True])
@pytest.mark.parametrize("dims", [1, 7, 8, 9, 127, 128, 129, 768, 4096])
def test_pack_is_packbits_padded_to_the_pitch(la, dims, centred):
    X, c = rows(dims)
    c = c if centred else None
    got = la.pack_sign_bits(X, c)
    want = np.zeros((len(X), 16 * -(-dims // 128)), np.uint8)
    with np.errstate(invalid="ignore"):
        packed = np.packbits(X > (c if centred else 0), axis=1, bitorder="little")
    want[:, :packed.shape[1]] = packed
    assert got.shape == want.shape and (got == want).all()
    assert (bit_rows_ref.pack(X, c) == want).all()  # the restatement the GPU tests use agrees with both


def test_symbols_and_refusals(la):
    L = la.lib()
    assert all(hasattr(L, name) and name in la._native.SIGNATURES for name in NAMES)
    with pytest.raises(la.LeannError) as e:
        la.pack_sign_bits(np.zeros((2, 4097), np.float32))
    assert e.value.code == 1 and "dims" in str(e.value)
    with pytest.raises(la.LeannError) as e:
        la.pack_sign_bits(np.zeros((2, 8), np.float32), np.zeros(7, np.float32))
    assert e.value.code == 1 and "centre" in str(e.value)
