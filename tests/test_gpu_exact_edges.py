"""-m gpu: the exact scan, the allow-bitmap compaction and the cross-shard merge (csrc/scan.hip) at the shapes the other suites
never launch: score_mfma_kernel in its general form (dims no multiple of 32, strides no multiple of 4, padded rows, bases off 16
bytes) with and without candidate emission and a row list, the repeat on the slab path after an overflow, top-k lists that hold
negative and large scores, bitmaps that end inside a byte or next to a block boundary, and the merge in descending order, above
64 KiB of LDS, at its limit and with 64-bit keys.

Everything is exact: keys equal, scores equal as uint32, counts equal, the unused tail UINT64_MAX with -inf (+inf for
distances).  Scores are held to po.scan_topk(mode=1), the k-ordered fmaf chain the kernel claims to reproduce bit for bit."""
import ctypes as C

import numpy as np
import pytest

from merge_ref import merge_ref
from test_gpu_filtered import _exact_oracle
from util import SEED, synth

pytestmark = pytest.mark.gpu

U64MAX = np.iinfo(np.uint64).max
NEG_INF, POS_INF = 0xFF800000, 0x7F800000
GUARD = 64  # NaN floats in front of and behind every device image (a multiple of 4: the 16-byte alignment of the base is kept)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _pack(allowed):
    return np.packbits(allowed, bitorder="little")


class Scan:
    """leann_scan_topk_device over host arrays laid out so that every read outside the data shows: rows in a NaN-filled image
    [n + 1, ld] (pad columns [dims, ld) and one row behind the last are NaN), queries in the middle of a NaN-filled buffer, both
    between NaN guards.  x_shift / q_shift move a base by that many floats off its 16-byte alignment."""

    def __init__(self, la, X, Q, ld=None, x_shift=0, q_shift=0):
        self.la, self.X, self.Q = la, X, Q
        self.n, self.d = X.shape
        self.nq, self.ld = len(Q), ld or self.d
        img = np.full((self.n + 1, self.ld), np.nan, np.float32)
        img[: self.n, : self.d] = X
        flat = np.full(GUARD + x_shift + img.size + GUARD, np.nan, np.float32)
        flat[GUARD + x_shift: GUARD + x_shift + img.size] = img.ravel()
        qflat = np.full(GUARD + q_shift + Q.size + GUARD, np.nan, np.float32)
        qflat[GUARD + q_shift: GUARD + q_shift + Q.size] = Q.ravel()
        self.dX, self.dQ = la.DeviceArray.from_host(flat), la.DeviceArray.from_host(qflat)
        assert self.dX.ptr % 16 == 0 and self.dQ.ptr % 16 == 0
        self.xptr, self.qptr = self.dX.ptr + 4 * (GUARD + x_shift), self.dQ.ptr + 4 * (GUARD + q_shift)

    def run(self, k, mask=None, key_offset=0, n=None, nq=None):
        la, n, nq = self.la, self.n if n is None else n, self.nq if nq is None else nq
        dM = la.DeviceArray.from_host(mask) if mask is not None else None
        dk, ds, dc = la.DeviceArray((nq, k), np.uint64), la.DeviceArray((nq, k), np.float32), la.DeviceArray(nq, np.uint32)
        la._native.check(la.lib().leann_scan_topk_device(self.xptr, n, self.d, self.ld, self.qptr, nq, k, dM.ptr if dM else None, key_offset,
                                                         dk.ptr, ds.ptr, dc.ptr, None))
        la.sync()
        return dk.to_host(), ds.to_host(), dc.to_host()


def _reference(po, X, Q, k, mask=None, queries=None):
    """-> {query: (keys, scores)} of po.scan_topk(mode=1), computed once per case"""
    return {i: po.scan_topk(X, Q[i], k, mode=1, allow_mask=mask) for i in (range(len(Q)) if queries is None else queries)}


def _same(ref, got, k, key_offset=0):
    gk, gs, gc = got
    for i, (rk, rs) in ref.items():
        m = len(rk)
        assert int(gc[i]) == m, f"query {i}: count {gc[i]} != {m}"
        assert (gk[i, :m] == rk + np.uint64(key_offset)).all(), f"query {i}: keys differ at {np.nonzero(gk[i, :m] != rk + np.uint64(key_offset))[0][:5]}"
        assert (_bits(gs[i, :m]) == _bits(rs)).all(), f"query {i}: score bits differ"
        assert (gk[i, m:] == U64MAX).all() and (_bits(gs[i, m:]) == NEG_INF).all(), f"query {i}: tail"


def _same_runs(a, b):
    assert (a[0] == b[0]).all() and (_bits(a[1]) == _bits(b[1])).all() and (a[2] == b[2]).all()


def _slab_path(la, monkeypatch, on):
    if on:
        monkeypatch.setenv("LEANN_DEBUG_NO_EMIT", "1")
    else:
        monkeypatch.delenv("LEANN_DEBUG_NO_EMIT")
    la.lib().leann_debug_reload_env()


# ---- 1. score_mfma_kernel<LIST=false, FAST=false> on the slab path (n <= 65536) ---------------------------------------------

LAYOUTS = [  # dims, ld, x_shift, q_shift
    pytest.param(1, 1, 0, 0, id="d1-scalar-all-ties"),        # every score is +-1: the order within a sign is the position alone
    pytest.param(3, 3, 0, 0, id="d3-scalar"),
    pytest.param(31, 31, 0, 0, id="d31-scalar"),
    pytest.param(33, 33, 0, 0, id="d33-scalar-two-ktiles"),
    pytest.param(100, 100, 0, 0, id="d100-vector-partial-ktile"),
    pytest.param(260, 260, 0, 0, id="d260-vector-partial-ktile"),
    pytest.param(100, 104, 0, 0, id="d100-ld104-padded-vector"),
    pytest.param(64, 67, 0, 0, id="d64-ld67-stride-off-fast"),
    pytest.param(64, 64, 1, 0, id="d64-rows-plus-4-bytes"),     # xvec false, qvec true
    pytest.param(64, 64, 0, 1, id="d64-queries-plus-4-bytes"),  # qvec false, xvec true
    pytest.param(96, 100, 0, 0, id="d96-ld100-fast-control"),   # FAST with ld != dims
]


@pytest.mark.parametrize("d,ld,x_shift,q_shift", LAYOUTS)
def test_general_score_kernel_layouts(la, po, gpu, d, ld, x_shift, q_shift):
    n, nq, k = 2049, 5, 10
    X, Q = synth(po, n, d), synth(po, nq, d, stream=1)
    if d == 1:
        assert set(np.abs(X).ravel().tolist()) == {1.0}
    s = Scan(la, X, Q, ld, x_shift, q_shift)
    _same(_reference(po, X, Q, k), s.run(k), k)


TILE_EDGES = [  # n, nq, k: every n of {1, 127, 128, 129, 2047, 2048, 2049, 4097}, every nq of {1, 63, 64, 65, 130}, k of {1, 10, 1024}
    (1, 1, 1), (127, 63, 10), (128, 64, 10), (129, 65, 10), (2047, 1, 1024), (2048, 63, 1), (2049, 130, 10), (4097, 64, 1024),
    (4097, 65, 10), (129, 130, 1), (1, 130, 10), (2048, 5, 1024),
    (600, 3, 1024),  # k > n
]


@pytest.mark.parametrize("n,nq,k", TILE_EDGES)
def test_general_score_kernel_tile_edges(la, po, gpu, n, nq, k):
    """dims 33 in rows of 36: a 1-column last k-tile, vector loads that must stop at column 32 (the rest of the row is NaN)"""
    d, ld = 33, 36
    X, Q = synth(po, n, d), synth(po, nq, d, stream=1)
    ref = _reference(po, X, Q, k)
    assert all(len(rk) == min(n, k) for rk, _ in ref.values())
    _same(ref, Scan(la, X, Q, ld).run(k), k)


def test_general_score_kernel_k_above_n_keeps_position_order(la, po, gpu):
    """n = 5, k = 10, dims = 1: the five entries of a sign come back in position order, then the tail"""
    X, Q = synth(po, 5, 1), synth(po, 3, 1, stream=1)
    ref = _reference(po, X, Q, 10)
    got = Scan(la, X, Q).run(10)
    _same(ref, got, 10)
    for i in range(3):
        sc = X[:, 0] * Q[i, 0]
        want = np.concatenate([np.nonzero(sc > 0)[0], np.nonzero(sc < 0)[0]])
        assert (got[0][i, :5] == want.astype(np.uint64)).all() and got[2][i] == 5


def test_general_score_kernel_allow_mask(la, po, gpu):
    n, d, nq, k = 2049, 100, 5, 10
    X, Q = synth(po, n, d), synth(po, nq, d, stream=1)
    s = Scan(la, X, Q)
    third = _pack(np.arange(n) % 3 == 0)
    _same(_reference(po, X, Q, k, third), s.run(k, third), k)
    few = np.zeros(n, bool)
    few[[0, 130, 131, 1029, 2047, 2048]] = True  # fewer allowed rows than k
    ref = _reference(po, X, Q, k, _pack(few))
    assert all(len(rk) == 6 for rk, _ in ref.values())
    _same(ref, s.run(k, _pack(few)), k)


# ---- 2. the general form with candidate emission (more than 65536 rows), and the repeat after an overflow --------------------

def test_general_score_kernel_emission(la, po, gpu, monkeypatch):
    """<false, false> with CandEmit, with and without a mask, against the oracle and against its own slab path; rows 65535 and 65536
    (the last of the first slab, the first emitted one) tie with query 0's best row: the lower position comes first.
    What this cannot tell apart is `>=` from `>` in the kernel's emission test: a later row that only ties the running k-th best ranks
    behind the k earlier rows that set it, so dropping it changes candidate counts and no result.  A threshold that is too HIGH (one
    rank, say) does fail here: 29 of the 70 queries have a winner behind the first slab."""
    n, d, nq, k, off = 70001, 100, 70, 10, 7
    X, Q = synth(po, n, d).copy(), synth(po, nq, d, stream=1)
    best = int(po.scan_topk(X, Q[0], 1, mode=1)[0][0])
    assert best < 65535
    X[65535] = X[65536] = X[best]
    mask = _pack(np.arange(n) % 3 == 1)   # 65536 % 3 == 1: the emitted twin is allowed, its neighbour in the slab is not
    s = Scan(la, X, Q)
    spot = (0, 31, 32, 69)
    ref, refm = _reference(po, X, Q, k, queries=spot), _reference(po, X, Q, k, mask, queries=spot)
    assert ref[0][0][:3].tolist() == [best, 65535, 65536] and len(set(_bits(ref[0][1][:3]).tolist())) == 1
    assert refm[0][0][:2].tolist() == ([best, 65536] if best % 3 == 1 else [65536, int(refm[0][0][1])])
    plain, masked = s.run(k, key_offset=off), s.run(k, mask, key_offset=off)
    _same(ref, plain, k, off)
    _same(refm, masked, k, off)
    _slab_path(la, monkeypatch, True)
    _same_runs(s.run(k, key_offset=off), plain)
    _same_runs(s.run(k, mask, key_offset=off), masked)
    _slab_path(la, monkeypatch, False)


def test_general_score_kernel_overflow_repeats_on_slabs(la, po, gpu):
    """scores that rise with the position: more rows behind the first slab reach its 10th-best score than a candidate list holds, the
    call repeats on the slab path"""
    n, d, nq, k = 80000, 20, 3, 10
    X, Q = synth(po, n, d), synth(po, nq, d, stream=1)
    keys, sc = po.scan_topk(X, Q[0], n, mode=1)
    X = X[keys[::-1].astype(np.int64)]  # ascending by the chain score against query 0
    asc = sc[::-1]
    thr = np.sort(asc[:65536])[-k]
    survivors = int((asc[65536:] >= thr).sum())
    assert survivors > 8192, survivors  # EMIT_CAP
    ref = _reference(po, X, Q, k)
    assert ref[0][0].tolist() == list(range(n - 1, n - 1 - k, -1))
    got = Scan(la, X, Q).run(k)
    _same(ref, got, k)
    assert got[0][0].tolist() == list(range(n - 1, n - 1 - k, -1))


def test_list_score_kernel_emission(la, po, gpu):
    """<LIST=true, FAST=false> with CandEmit: an exact filtered search over 65625 listed rows of width 50"""
    n, d, ld, nq = 70000, 50, 52, 9
    X, Q = synth(po, n, d), synth(po, nq, d, stream=1)
    Xp = np.zeros((n, ld), np.float32)
    Xp[:, :d] = X
    dX = la.DeviceArray.from_host(Xp)
    s = la.BackendSearcher.build_device(la.BackendType.Hnsw, dX.ptr, n, d, ld, 8, 32)
    allowed = np.arange(n) % 16 != 0
    assert int(allowed.sum()) == 65625
    bm = _pack(allowed)
    for k in (1, 10, 100):
        ok, od, oc = _exact_oracle(po, X, Q, k, bm)
        gk, gd, gc = s.search_filtered_exact_batch(Q, k, bm)
        assert (gc == oc).all() and (gk == ok).all() and (_bits(gd) == _bits(od)).all()
    s.close()


# ---- 3. sign and magnitude of the scores in a top-k ---------------------------------------------------------------------------

def test_topk_crosses_zero(la, po, gpu):
    n, d, nq, k = 600, 100, 5, 512
    X, Q = synth(po, n, d), synth(po, nq, d, stream=1)
    ref = _reference(po, X, Q, k)
    for rk, rs in ref.values():
        assert (rs > 0).sum() >= 50 and (rs < 0).sum() >= 50  # both halves of f32_orderable in one list
    _same(ref, Scan(la, X, Q).run(k), k)


def test_topk_all_scores_negative(la, po, gpu):
    n, d, nq, k = 2049, 100, 5, 10
    X, Q = -np.abs(synth(po, n, d)), np.abs(synth(po, nq, d, stream=1))
    ref = _reference(po, X, Q, k)
    assert all((rs < 0).all() for _, rs in ref.values())
    _same(ref, Scan(la, X, Q).run(k), k)


def test_topk_scaled_rows(la, po, gpu):
    """rows scaled by 2^-40 .. 2^40 (exact), every second one negated: winners near 1e11, losers near -1e11"""
    n, d, nq, k = 3000, 100, 5, 20
    rng = np.random.default_rng(3000)
    scale = np.ldexp(np.float32(1), rng.integers(-40, 41, n)).astype(np.float32)
    scale[1::2] *= -1
    X, Q = synth(po, n, d) * scale[:, None], synth(po, nq, d, stream=1)
    ref = _reference(po, X, Q, k)
    full = po.scan_topk(X, Q[0], n, mode=1)[1]
    assert np.isfinite(full).all() and full[0] > 1e9 and full[-1] < -1e9
    assert all(np.isfinite(rs).all() for _, rs in ref.values())
    _same(ref, Scan(la, X, Q).run(k), k)


# ---- 4. allow-bitmap compaction (allow_count_kernel, allow_offsets_kernel, allow_scatter_kernel) -------------------------------

@pytest.mark.parametrize("n", [8191, 8192, 8193, 16385, 1001])
def test_allow_compaction_edges(la, po, gpu, n):
    """a block of the compaction covers 8192 positions, a thread 32, a byte 8: n on both sides of each, single bits at the ends and
    around the block boundary, and stray bits behind n in the last byte, which the host wrapper passes on and the kernels must
    mask (allow_word)"""
    d, nq, k = 16, 5, 10
    rng = np.random.default_rng(n)
    X, Q = synth(po, n, d), synth(po, nq, d, stream=1)
    dX = la.DeviceArray.from_host(X)
    s = la.BackendSearcher.build_device(la.BackendType.Hnsw, dX.ptr, n, d, d, 8, 32)
    cases = {"ones": np.ones(n, bool), "first": np.arange(n) == 0, "last": np.arange(n) == n - 1,
             "boundary": np.isin(np.arange(n), [8190, 8191, 8192, 8193]), "random": rng.random(n) < 0.5}
    assert int(cases["boundary"].sum()) == min(4, max(0, n - 8190))
    for name, allowed in cases.items():
        clean = _pack(allowed)
        variants = [clean]
        if n % 8:
            stray = clean.copy()
            stray[-1] |= np.uint8((0xFF << (n % 8)) & 0xFF)
            variants.append(stray)
        ok, od, oc = _exact_oracle(po, X, Q, k, clean)
        assert (oc == min(k, int(allowed.sum()))).all()
        for bm in variants:
            f = s.register_filter(bm)
            assert f.count() == int(allowed.sum()), name
            f.close()
            gk, gd, gc = s.search_filtered_exact_batch(Q, k, bm)
            assert (gc == oc).all() and (gk == ok).all() and (_bits(gd) == _bits(od)).all(), name
    s.close()


# ---- 5. merge_topk_kernel ------------------------------------------------------------------------------------------------------

def _lists(rng, S, nq, k_in, values, descending, keys):
    """[S, nq, k_in] lists as a shard returns them: sorted by (score descending | dist ascending, key ascending)"""
    keys = keys.reshape(S, nq, k_in).copy()
    vals = rng.choice(np.asarray(values, np.float32), (S, nq, k_in))
    for s in range(S):
        for q in range(nq):
            o = np.lexsort((keys[s, q], -vals[s, q] if descending else vals[s, q]))
            keys[s, q], vals[s, q] = keys[s, q][o], vals[s, q][o]
    return keys, vals


def _merge(la, keys, vals, counts, k_out, descending):
    S, nq, k_in = keys.shape
    dk, dd, dc = la.DeviceArray.from_host(keys), la.DeviceArray.from_host(vals), la.DeviceArray.from_host(counts)
    ok, od, oc = la.DeviceArray((nq, k_out), np.uint64), la.DeviceArray((nq, k_out), np.float32), la.DeviceArray(nq, np.uint32)
    la._native.check(la.lib().leann_merge_topk_device(dk.ptr, dd.ptr, dc.ptr, S, nq, k_in, k_out, descending, ok.ptr, od.ptr, oc.ptr, None))
    la.sync()
    return ok.to_host(), od.to_host(), oc.to_host()


def _merge_same(got, want, k_out, descending):
    gk, gd, gc = got
    for q, (rk, rd) in enumerate(want):
        m = len(rk)
        assert int(gc[q]) == m, q
        assert (gk[q, :m] == rk).all() and (_bits(gd[q, :m]) == _bits(rd)).all(), q
        assert (gk[q, m:] == U64MAX).all() and (_bits(gd[q, m:]) == (NEG_INF if descending else POS_INF)).all(), q


TIED_SCORES = [-3.0, -1.5, -0.75, -0.25, 0.5]  # mostly negative: the best few of a query reach below zero


@pytest.mark.parametrize("k_out", [10, 4, 25])
def test_merge_descending_matches_reference(la, gpu, k_out):
    S, nq, k_in = 8, 33, 10
    rng = np.random.default_rng(50 + k_out)
    keys, sc = _lists(rng, S, nq, k_in, TIED_SCORES, True, rng.permutation(S * nq * k_in).astype(np.uint64))
    counts = rng.integers(0, k_in + 1, (S, nq)).astype(np.uint32)
    counts[:, 17] = 0                       # one query without any entry
    counts[:, 3] = k_in                     # one with every list full
    for s in range(S):                      # one with negative scores only
        v = -np.abs(sc[s, 5])
        o = np.lexsort((keys[s, 5], -v))
        keys[s, 5], sc[s, 5] = keys[s, 5][o], v[o]
    counts[0, 5] = k_in
    got = _merge(la, keys, sc, counts, k_out, 1)
    want = [merge_ref(keys[:, q], sc[:, q], counts[:, q], k_out, descending=True) for q in range(nq)]
    assert len(want[17][0]) == 0 and len(want[3][0]) == min(k_out, S * k_in)
    assert len(want[5][1]) == min(k_out, int(counts[:, 5].sum())) >= 4 and (want[5][1] < 0).all()
    assert any(len(set(rd.tolist())) < len(rd) for _, rd in want)  # ties decide
    _merge_same(got, want, k_out, True)


def test_merge_ascending_with_64_bit_keys(la, po, gpu):
    S, nq, k_in, k_out = 8, 33, 10, 10
    rng = np.random.default_rng(64)
    raw = rng.integers(1 << 40, 1 << 63, S * nq * k_in, dtype=np.uint64)
    assert len(np.unique(raw)) == len(raw) and (raw >> np.uint64(32)).min() > 0
    keys, dists = _lists(rng, S, nq, k_in, [-2.0, -0.5, 0.125, 0.75, 1.0, np.inf], False, raw)
    counts = rng.integers(0, k_in + 1, (S, nq)).astype(np.uint32)
    counts[:, 0] = k_in
    got = _merge(la, keys, dists, counts, k_out, 0)
    want = [po.merge_topk(keys[:, q], dists[:, q], counts[:, q], k_out) for q in range(nq)]
    for q in range(nq):  # the numpy reference agrees with the oracle on these inputs too
        rk, rd = merge_ref(keys[:, q], dists[:, q], counts[:, q], k_out)
        assert (rk == want[q][0]).all() and (_bits(rd) == _bits(want[q][1])).all()
    _merge_same(got, want, k_out, False)
    # +inf as the distance of a valid entry: a query whose lists hold nothing else keeps its keys
    dists[:, 1] = np.inf
    for s in range(S):
        keys[s, 1] = np.sort(keys[s, 1])
    counts[:, 1] = 2
    got = _merge(la, keys, dists, counts, 25, 0)
    want = [po.merge_topk(keys[:, q], dists[:, q], counts[:, q], 25) for q in range(nq)]
    assert len(want[1][0]) == 2 * S and np.isinf(want[1][1]).all()
    _merge_same(got, want, 25, False)


def test_merge_large_lds_and_limit(la, po, gpu):
    """12 x 1024 = 12288 entries (144 KiB of dynamic LDS, above the 64 KiB a kernel gets unasked) in both orders, then a small merge
    in the same process under the raised function attribute; one shard more is refused and writes nothing"""
    S, nq, k_in, k_out = 12, 3, 1024, 1024
    rng = np.random.default_rng(12288)
    values = (np.arange(-40, 41, dtype=np.float32) + 0.5) / 8  # 81 values for 12288 entries: ties everywhere, no zero
    for descending in (0, 1):
        keys, vals = _lists(rng, S, nq, k_in, values, bool(descending), rng.permutation(S * nq * k_in).astype(np.uint64) + np.uint64(1 << 33))
        counts = np.array([[k_in] * nq] * S, np.uint32)
        counts[:, 1] = rng.integers(0, k_in + 1, S)
        got = _merge(la, keys, vals, counts, k_out, descending)
        if descending:
            want = [merge_ref(keys[:, q], vals[:, q], counts[:, q], k_out, descending=True) for q in range(nq)]
        else:
            want = [po.merge_topk(keys[:, q], vals[:, q], counts[:, q], k_out) for q in range(nq)]
        _merge_same(got, want, k_out, bool(descending))
    keys, vals = _lists(rng, 2, 4, 5, TIED_SCORES, False, rng.permutation(40).astype(np.uint64))
    counts = rng.integers(0, 6, (2, 4)).astype(np.uint32)
    _merge_same(_merge(la, keys, vals, counts, 5, 0), [po.merge_topk(keys[:, q], vals[:, q], counts[:, q], 5) for q in range(4)], 5, False)
    # 13 x 1024 = 12289 ... 13312 entries: over the limit
    S = 13
    dk, dd = la.DeviceArray.from_host(np.zeros((S, nq, k_in), np.uint64)), la.DeviceArray.from_host(np.zeros((S, nq, k_in), np.float32))
    dc = la.DeviceArray.from_host(np.full((S, nq), k_in, np.uint32))
    fill_k, fill_d, fill_c = np.full((nq, k_out), 0x1234, np.uint64), np.full((nq, k_out), 7.5, np.float32), np.full(nq, 99, np.uint32)
    ok, od, oc = la.DeviceArray.from_host(fill_k), la.DeviceArray.from_host(fill_d), la.DeviceArray.from_host(fill_c)
    rc = la.lib().leann_merge_topk_device(dk.ptr, dd.ptr, dc.ptr, S, nq, k_in, k_out, 0, ok.ptr, od.ptr, oc.ptr, None)
    la.sync()
    assert rc == 1  # LEANN_ERR_INVALID
    assert (ok.to_host() == fill_k).all() and (od.to_host() == fill_d).all() and (oc.to_host() == fill_c).all()


def test_merge_limit_is_on_entries(la, gpu):
    """the refusal is at 12289 entries, not at 13 shards: 12289 lists of one entry"""
    S, nq = 12289, 1
    dk, dd = la.DeviceArray.from_host(np.zeros((S, nq, 1), np.uint64)), la.DeviceArray.from_host(np.zeros((S, nq, 1), np.float32))
    dc = la.DeviceArray.from_host(np.ones((S, nq), np.uint32))
    ok, od, oc = la.DeviceArray.from_host(np.full((1, 1), 5, np.uint64)), la.DeviceArray.from_host(np.full((1, 1), 5, np.float32)), \
        la.DeviceArray.from_host(np.full(1, 5, np.uint32))
    assert la.lib().leann_merge_topk_device(dk.ptr, dd.ptr, dc.ptr, S, nq, 1, 1, 0, ok.ptr, od.ptr, oc.ptr, None) == 1
    la.sync()
    assert ok.to_host()[0, 0] == 5 and od.to_host()[0, 0] == 5 and oc.to_host()[0] == 5


# ---- 6. query projection (leann_internal_score over the encoder weights) at widths off the fast path --------------------------

@pytest.mark.parametrize("d", [pytest.param(200, id="d200-vector-general"), pytest.param(90, id="d90-scalar-general")])
def test_recompute_on_graph_projection_off_the_fast_path(la, po, gpu, d):
    """part (a) of test_recompute_on_graph_search at dims no multiple of 32: W q is computed by <false, false> with ld = dims"""
    n, h, nq, k = 3000, 64, 40, 10
    Lc, chk = la.lib(), la._native.check
    F = po.synth_features(SEED, h, 64, 1.0, 0, 0, n)
    W = po.synth_weights(SEED, h, d)
    Q = po.recompute_encode(po.synth_features(SEED, h, 64, 1.0, 1, 0, nq), W)
    dF, dW = la.DeviceArray.from_host(F), la.DeviceArray.from_host(W)
    r = C.c_void_p()
    chk(Lc.leann_recompute_create(dF.ptr, n, h, dW.ptr, d, 0, 0, C.byref(r)))
    hb = C.c_void_p()
    chk(Lc.leann_recompute_build_index(r, 0, 16, 64, C.byref(hb)))
    s = la.BackendSearcher(hb, la.BackendType.Hnsw)
    fh, rb = C.c_uint32(0), C.c_uint32(0)
    chk(Lc.leann_backend_feature_rows_export(hb, C.byref(fh), C.byref(rb), None))
    assert fh.value == h
    rows = np.zeros((n, rb.value), np.uint8)
    chk(Lc.leann_backend_feature_rows_export(hb, None, None, rows.ctypes.data))
    s.stats(reset=True)
    gk, gd, gc = s.search_batch(Q, k, 64)
    st = s.stats()
    g = s.graph_export()
    Gr = po.Graph.from_arrays(np.zeros((n, 1), np.float32), 16, 32, g["max_level"], g["entry"], g["levels"], g["upper_off"], g["adj0"], g["adjU"])
    Gr.set_features(rows, fh.value, rb.value)
    ok, od, oc, ost = Gr.search_batch(po.project_queries(W, Q, fh.value), k, 64, 0, 8)
    assert (gc == oc).all() and (gk == ok).all() and (_bits(gd) == _bits(od)).all()
    assert st["n_dist_evals"] == int(ost[:, 0].sum())
    s.close()
    Lc.leann_recompute_close(r)
