"""CPU suite: the flat search on bf16 rows (include/leann_backend.h "exhaustive search on bf16 rows") — the host split twin
leann_split_query_bf16 against tests/flat_bf16_ref.py.  The device's pieces are not exposed; tests/test_gpu_flat_bf16.py holds them
through the order-free equalities."""
import numpy as np

import flat_bf16_ref


def test_split_query_is_the_restatement_and_reproduces_the_query(la):
    rng = np.random.default_rng(5)
    q = (rng.standard_normal(4099) * np.exp2(rng.integers(-40, 40, 4099))).astype(np.float32)
    q[:6] = [0.0, -0.0, 1 + 2.0 ** -10, 1 - 2.0 ** -10, 1 + 2.0 ** -8, 2.0 ** -8 + 2.0 ** -17]  # exact, hi = 1, a tie to even, lo a tie
    hi, lo = la.split_query_bf16(q)
    rhi, rlo = flat_bf16_ref.split(q)
    assert (hi == rhi).all() and (lo == rlo).all() and (hi == la.round_bf16(q)).all()
    back = flat_bf16_ref.widen(hi).astype(np.float64) + flat_bf16_ref.widen(lo).astype(np.float64)
    assert (np.abs(back - q.astype(np.float64)) <= 2.0 ** -17 * np.abs(q.astype(np.float64))).all()
    assert hi[2] == hi[3] == 0x3F80 and flat_bf16_ref.widen(lo[2:4]).tolist() == [2.0 ** -10, -2.0 ** -10]
