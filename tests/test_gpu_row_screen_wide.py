"""-m gpu: the wide form of the row screen's phase C (search.cuh, beam_search_screen_kernel<3, 4>): one hi-plane round over H rows per
wave, then the survivors read as whole rows, 4 at a time; hops of an unfilled beam skip the hi round.  test_gpu_row_screen.py builds
M = 16 graphs, whose lists hold at most 32 ids: one wide round, never full.  Here M = 32 — level-0 lists of 64 ids, so hops of more than
one wide round and hops at and just past 4 * H rows — and the same bar: ids, distance bits, counts and stats equal with the screen on,
with it off, and in the oracle walking the exported graph; the device's ruled-out total equal to the oracle's count on the same walk
(_same_as_oracle); ruled out + read in full = every evaluation but the entry points'."""
import numpy as np
import pytest

from test_gpu_row_screen import NQ, _on_off, _same, _same_as_oracle
from util import SEED, synth

pytestmark = pytest.mark.gpu

M = 32


def _built(la, po, X):
    n, d = X.shape
    dX = la.DeviceArray.from_host(X)
    s = la.BackendSearcher.build_device(la.BackendType.Hnsw, dX.ptr, n, d, d, M, 64)
    g = s.graph_export()
    G = po.Graph.from_arrays(X, M, 2 * M, g["max_level"], g["entry"], g["levels"], g["upper_off"], g["adj0"], g["adjU"])
    return s, G, dX


# 520: plane rows of 576 (one interleaved block + a 64-element tail): the survivor pass reads the tail chunk of both planes again
@pytest.fixture(scope="module", params=[768, 520])
def clustered(request, la, po, gpu):
    d = request.param
    X = synth(po, 4000, d, n_clusters=2)
    Q = synth(po, NQ, d, stream=1, n_clusters=2)
    s, G, dX = _built(la, po, X)
    yield s, G, Q
    s.close()


# 600: the beam takes most of the search to fill, and a hop of an unfilled beam rules nothing out (the share printed shows it)
@pytest.mark.parametrize("ef", [10, 56, 600])
def test_wide_screen_on_equals_off_equals_oracle(clustered, ef):
    s, G, Q = clustered
    on, off = _on_off(s, Q, 10, ef)
    evals = on["stats"]["n_dist_evals"] - NQ
    print(f"d={Q.shape[1]} M={M} ef={ef}: ruled out {on['ruled']} ({100.0 * on['ruled'] / evals:.1f} %), read in full {on['full']}, "
          f"evals {evals}, {evals / on['stats']['n_hops_base']:.1f} rows per level-0 hop")
    _same(on, off)
    _same_as_oracle(on, G, Q, 10, ef)
    assert on["ruled"] > 0
    assert on["ruled"] + on["full"] == evals
    assert off["ruled"] == 0 and off["full"] == 0


def test_near_duplicates_survive_more_than_four_per_wave(la, po, gpu):
    """The corpus of test_adversarial_rows_at_the_bound (near-duplicates of one direction, lower halves at the worst case of the
    truncation, a few zeros and subnormals) at M = 32: almost every row survives the hi round, so a wave regularly has more than 4
    survivors among its H rows and the survivor pass loops."""
    n, d = 2048, 768
    rng = np.random.default_rng(SEED)
    c = rng.standard_normal(d)
    c /= np.linalg.norm(c)

    def near(m):
        v = c + 1e-3 * rng.standard_normal((m, d))
        return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)

    X, Q = near(n), near(NQ)
    bits = X.view(np.uint32)
    same_sign = (bits >> 31).astype(bool) == (Q[0] < 0)[None, :]
    bits[:] = (bits & np.uint32(0xFFFF0000)) | np.where(same_sign, np.uint32(0xFFFF), np.uint32(0))
    for j, b in ((5, 0x00000000), (77, 0x80000000), (300, 0x0000FFFF), (511, 0x807FFFFF), (767, 0x0080FFFF)):
        bits[j::9, j] = np.uint32(b)
    s, G, dX = _built(la, po, X)
    for ef in (10, 56):
        on, off = _on_off(s, Q, 10, ef)
        print(f"near-duplicates M={M} ef={ef}: ruled out {on['ruled']}, read in full {on['full']}")
        _same(on, off)
        _same_as_oracle(on, G, Q, 10, ef)
        assert on["ruled"] + on["full"] == on["stats"]["n_dist_evals"] - NQ
        assert on["full"] > on["ruled"]  # not passed by ruling everything out
    s.close()
