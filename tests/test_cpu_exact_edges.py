"""CPU: the numpy merge reference (tests/merge_ref.py) against the oracle's k-way merge, without the code under test —
test_gpu_exact_edges.py then holds csrc/scan.hip: merge_topk_kernel to it in the order the oracle does not have."""
import numpy as np
import pytest

from merge_ref import f32_orderable, merge_ref

U64MAX = np.iinfo(np.uint64).max


def tied_lists(rng, S, k_in, values, descending, key_lo=0, key_hi=1 << 20):
    """S lists of k_in unique keys with values from a small set (many ties), each sorted the way a shard returns it"""
    keys = rng.choice(np.arange(key_lo, key_hi, dtype=np.uint64), S * k_in, replace=False).reshape(S, k_in)
    vals = rng.choice(np.asarray(values, np.float32), (S, k_in))
    for s in range(S):
        o = np.lexsort((keys[s], -vals[s] if descending else vals[s]))
        keys[s], vals[s] = keys[s][o], vals[s][o]
    return keys, vals


VALUES = [-2.5, -1.0, -0.125, 0.125, 0.5, 1.0, 3.0, np.inf]


def test_f32_orderable_orders_like_the_floats():
    x = np.array([-np.inf, -3e38, -1.0, -1e-30, 1e-30, 0.5, 1.0, 3e38, np.inf], np.float32)
    o = f32_orderable(x)
    assert (np.diff(o.astype(np.int64)) > 0).all()


@pytest.mark.parametrize("S,k_in,k_out", [(8, 10, 10), (8, 10, 4), (8, 10, 25), (1, 7, 7), (3, 1, 5), (12, 64, 100)])
def test_merge_ref_ascending_is_the_oracle_merge(po, S, k_in, k_out):
    rng = np.random.default_rng(S * 1000 + k_in * 10 + k_out)
    for trial in range(20):
        keys, dists = tied_lists(rng, S, k_in, VALUES, False)
        counts = rng.integers(0, k_in + 1, S).astype(np.uint32)
        if trial == 0:
            counts[:] = 0
        if trial == 1:
            counts[:] = k_in
        ok, od = po.merge_topk(keys, dists, counts, k_out)
        rk, rd = merge_ref(keys, dists, counts, k_out)
        assert len(rk) == len(ok) == min(int(counts.sum()), k_out)
        assert (rk == ok).all() and (rd.view(np.uint32) == od.view(np.uint32)).all()


def test_merge_ref_descending_mirrors_ascending():
    """descending over scores == ascending over the negated scores (negation is exact; the value set has no zero)"""
    rng = np.random.default_rng(77)
    for trial in range(20):
        keys, sc = tied_lists(rng, 8, 10, [-v for v in VALUES], True, key_lo=1 << 40, key_hi=(1 << 40) + 4096)
        counts = rng.integers(0, 11, 8).astype(np.uint32)
        dk, dv = merge_ref(keys, sc, counts, 25, descending=True)
        ak, av = merge_ref(keys, -sc, counts, 25)
        assert (dk == ak).all() and (dv.view(np.uint32) == (-av).view(np.uint32)).all()
        assert ((dv[1:] < dv[:-1]) | ((dv[1:] == dv[:-1]) & (dk[1:] > dk[:-1]))).all()
