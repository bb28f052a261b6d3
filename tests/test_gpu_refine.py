"""-m gpu: refining search results on exact f32 rows (include/leann_backend.h "refining results on exact rows", csrc/refine.hip).

The definition under test (tests/refine_ref.py restates it in numpy): the valid candidates of a list, scored with the distance the f32
traversal computes and ordered by (distance, key), first top_k.  Every comparison is bit for bit — keys, f32 distance bits, counts,
skipped counts — so there is no tolerance anywhere.

rerank_kernel<T, R> is compiled per row width T (chunks of 256 floats); one case per T:

    d      50   256   260   768   1024   1600   2048   2820   4096
    T       1     1     2     3      4      8      8     12     16
    R      16    16    16    16     13      6      6      3      2

(1 600 floats are 7 chunks and take the 8-chunk kernel with one chunk of zeros; 2 820 are 12 chunks with a partial last one.)  The
6-chunk kernel (R = 8), which none of these reaches, is run by d = 1 300 in test_width_six.  A workgroup of four waves takes one query:
each wave a contiguous quarter of the list in groups of R rows, so lists of 33 entries give the waves 9, 9, 9 and 6 candidates — more
than one group from T = 6 on, a partial group everywhere."""
import ctypes as C

import numpy as np
import pytest

import i8_ref
import refine_ref
from refine_ref import NO_KEY
from util import HipStreams, recall_at_k, synth

pytestmark = pytest.mark.gpu
INVALID = 1
M, EFC = 8, 48
NQ = 704  # > 512: the 4-wave walk on narrow rows; 64: the 16-wave one
POISON_K, POISON_D = 0xDEADBEEFDEADBEEF, 0xABABABAB
GUARD = 8  # words behind every output array


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rerank(la, rows, Q, keys, counts, top_k, stream=None, streams=None):
    """leann_rerank_batch_device on uploaded lists -> (keys, dists, counts, skipped); the outputs start out poisoned and carry guard
    words behind them, which must come back untouched"""
    nq, fetch_k = keys.shape
    dQ, dK, dC = la.DeviceArray.from_host(Q), la.DeviceArray.from_host(keys), la.DeviceArray.from_host(counts.astype(np.uint32))
    ok = la.DeviceArray.from_host(np.full(nq * top_k + GUARD, POISON_K, np.uint64))
    od = la.DeviceArray.from_host(np.full(nq * top_k + GUARD, POISON_D, np.uint32))
    oc = la.DeviceArray.from_host(np.full(nq + GUARD, POISON_D, np.uint32))
    sk = la.DeviceArray.from_host(np.full(nq + GUARD, POISON_D, np.uint32))
    la.sync()
    la.rerank_batch_device(rows, dQ.ptr, nq, dK.ptr, dC.ptr, fetch_k, top_k, ok.ptr, od.ptr, oc.ptr, sk.ptr, stream)
    if stream is not None:
        streams.synchronize(stream)
    la.sync()
    k, d, c, s = ok.to_host(), od.to_host(), oc.to_host(), sk.to_host()
    assert (k[nq * top_k:] == POISON_K).all() and (d[nq * top_k:] == POISON_D).all()
    assert (c[nq:] == POISON_D).all() and (s[nq:] == POISON_D).all()
    for a in (dQ, dK, dC, ok, od, oc, sk):
        a.free()
    return k[: nq * top_k].reshape(nq, top_k), d[: nq * top_k].view(np.float32).reshape(nq, top_k), c[:nq], s[:nq]


def _equal(got, want, what=""):
    gk, gd, gc, gs = got
    wk, wd, wc, ws = want
    assert (gc == wc).all(), f"{what}: counts"
    assert (gk == wk).all(), f"{what}: keys differ in {(gk != wk).any(axis=1).sum()} of {len(gk)} queries"
    assert (_bits(gd) == _bits(wd)).all(), f"{what}: distance bits"
    if gs is not None and ws is not None:
        assert (gs == ws).all(), f"{what}: skipped"


# ---- 1. widths and tails ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [50, 256, 260, 768, 1024, 1600, 2048, 2820, 4096])
def test_widths_and_tails(la, po, gpu, d):
    n, nq, fetch_k, top_k, off = 600, 33, 33, 10, 5000
    X, Q = synth(po, n, d), synth(po, nq, d, stream=1)
    ld = (d + 3) & ~3
    assert (X[:, 256 * ((ld - 1) // 256):] != 0).any()  # the last chunk that holds data holds some
    rng = np.random.default_rng(d)
    keys = (off + rng.integers(0, n, (nq, fetch_k))).astype(np.uint64)
    counts = np.full(nq, fetch_k, np.uint32)
    rows = la.ExactRows.from_host(X, key_offset=off)
    assert rows.len() == n and rows.placement() == "hbm"
    want = refine_ref.rerank(po, X, Q, keys, counts, top_k, key_offset=off)
    assert (want[2] == top_k).all() and (want[0] >= off).all()
    _equal(_rerank(la, rows, Q, keys, counts, top_k), want, f"d={d}")
    rows.close()


def test_width_six(la, po, gpu):
    """1 300 floats are 6 chunks: the one compiled width the issue's list of dims does not reach"""
    n, nq, d = 300, 9, 1300
    X, Q = synth(po, n, d), synth(po, nq, d, stream=1)
    keys = np.random.default_rng(6).integers(0, n, (nq, 40)).astype(np.uint64)
    counts = np.full(nq, 40, np.uint32)
    rows = la.ExactRows.from_host(X)
    _equal(_rerank(la, rows, Q, keys, counts, 10), refine_ref.rerank(po, X, Q, keys, counts, 10), "d=1300")
    rows.close()


# ---- 2. list edges at d = 260 -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(la, po, gpu):
    """600 x 260 with two identical rows, 33 queries, an f32 handle over an oracle graph at a key offset, and the rows three ways"""
    n, d, off = 600, 260, 70000
    X, Q = synth(po, n, d), synth(po, 33, d, stream=1)
    X[17] = X[5]  # a tie under different keys
    X.setflags(write=False)
    G = po.Graph.build_hnsw(X, M=M, efc=EFC)
    lv, uo, a0, aU = G.export()
    s = la.BackendSearcher.from_arrays(la.BackendType.Hnsw, X, M, 2 * M, G.max_level, G.entry, lv, uo, a0, aU, key_offset=off)
    made = dict(n=n, d=d, off=off, X=X, Q=Q, G=G, s=s, hbm=la.ExactRows.from_host(X, key_offset=off, placement="hbm"),
                host=la.ExactRows.from_host(X, key_offset=off, placement="host"))
    made["dev"] = la.ExactRows.from_device(s.device_rows_ptr(), n, d, s.graph_info()["ld"], key_offset=off, keep=s)
    yield made
    for k in ("dev", "host", "hbm", "s"):
        made[k].close()


def _edge_lists(c, fetch_k, seed):
    """33 lists: random keys with out-of-range ones and the tail value inside the counted prefix, duplicates, the tied pair; counts 0,
    1, few, equal to fetch_k and above it"""
    n, off = c["n"], c["off"]
    rng = np.random.default_rng(seed)
    keys = (off + rng.integers(0, n, (33, fetch_k))).astype(np.uint64)
    bad = np.array([off - 1, off + n, off + n + 12345, 1 << 40, 3, NO_KEY, NO_KEY - 1], np.uint64)
    hit = rng.random(keys.shape) < 0.12
    keys[hit] = bad[rng.integers(0, len(bad), int(hit.sum()))]
    if fetch_k >= 2:
        keys[4, :2] = [off + 17, off + 5]            # the identical rows: the lower key must come first
        keys[5, : min(fetch_k, 4)] = off + 123       # one key listed again and again
    keys[6, :] = NO_KEY                               # nothing valid at all
    counts = rng.integers(0, fetch_k + 1, 33).astype(np.uint32)
    counts[:4] = [0, 1, max(fetch_k // 3, 1), fetch_k]
    counts[4:8] = fetch_k
    counts[8:12] = [fetch_k + 1, fetch_k + 5, 1 << 20, 0xFFFFFFFF]  # above fetch_k: clamped
    return keys, counts


@pytest.mark.parametrize("fetch_k", [1, 2, 33, 64, 1024])
def test_list_edges(la, po, small, fetch_k):
    c = small
    keys, counts = _edge_lists(c, fetch_k, fetch_k)
    full = refine_ref.rerank(po, c["X"], c["Q"], keys, counts, fetch_k, key_offset=c["off"])
    assert full[3].sum() > 0  # some keys were skipped and counted
    for top_k in sorted({1, fetch_k}):
        want = (full[0][:, :top_k], full[1][:, :top_k], np.minimum(full[2], top_k), full[3])  # the first top_k of the same order
        got = _rerank(la, c["hbm"], c["Q"], keys, counts, top_k)
        _equal(got, want, f"fetch_k={fetch_k} top_k={top_k}")
        gk, gd, gc, _ = got
        for q in range(33):  # the unused tail, written by the kernel over the poison
            assert (gk[q, gc[q]:] == NO_KEY).all() and (_bits(gd[q, gc[q]:]) == 0x7F800000).all()
        assert gc[0] == 0 and gc[6] == 0 and got[3][6] == fetch_k
    if fetch_k >= 2:
        row, lo, hi = full[0][4].tolist(), c["off"] + 5, c["off"] + 17  # the identical rows: equal distance bits, the lower key first
        assert lo in row and hi in row and max(i for i, k in enumerate(row) if k == lo) < row.index(hi)
        assert _bits(full[1][4, row.index(lo)]) == _bits(full[1][4, row.index(hi)])
        assert (full[0][5] == c["off"] + 123).sum() >= min(fetch_k, 4)  # a duplicated key is returned as often as it is listed


def test_one_query_per_call_leaves_the_next_row_alone(la, po, small):
    """nq = 1 into every other row of a larger buffer: the row behind each output row is a guard"""
    c = small
    fetch_k, top_k = 33, 10
    keys, counts = _edge_lists(c, fetch_k, 99)
    want = refine_ref.rerank(po, c["X"], c["Q"], keys, counts, top_k, key_offset=c["off"])
    dQ, dK, dC = la.DeviceArray.from_host(c["Q"]), la.DeviceArray.from_host(keys), la.DeviceArray.from_host(counts)
    ok = la.DeviceArray.from_host(np.full((66, top_k), POISON_K, np.uint64))
    od = la.DeviceArray.from_host(np.full((66, top_k), POISON_D, np.uint32))
    oc = la.DeviceArray.from_host(np.full(66, POISON_D, np.uint32))
    la.sync()
    for q in range(33):
        la.rerank_batch_device(c["hbm"], dQ.ptr + q * c["d"] * 4, 1, dK.ptr + q * fetch_k * 8, dC.ptr + q * 4, fetch_k, top_k,
                               ok.ptr + 2 * q * top_k * 8, od.ptr + 2 * q * top_k * 4, oc.ptr + 2 * q * 4)
    la.sync()
    k, d, cnt = ok.to_host(), od.to_host(), oc.to_host()
    assert (k[1::2] == POISON_K).all() and (d[1::2] == POISON_D).all() and (cnt[1::2] == POISON_D).all()
    _equal((k[0::2], d[0::2].view(np.float32), cnt[0::2], None), want, "one query per call")
    for a in (dQ, dK, dC, ok, od, oc):
        a.free()


# ---- 3. placements, streams ---------------------------------------------------------------------------------------------------------
def test_placements_return_identical_bytes(la, po, small):
    c = small
    assert c["hbm"].placement() == "hbm" and c["host"].placement() == "host" and c["dev"].placement() == "hbm"
    for fetch_k, top_k in ((33, 10), (1024, 1024)):
        keys, counts = _edge_lists(c, fetch_k, 7)
        a = _rerank(la, c["hbm"], c["Q"], keys, counts, top_k)
        for name in ("host", "dev"):
            b = _rerank(la, c[name], c["Q"], keys, counts, top_k)
            for x, y in zip(a, b):
                assert x.tobytes() == y.tobytes(), (name, fetch_k)
    _equal(a, refine_ref.rerank(po, c["X"], c["Q"], keys, counts, 1024, key_offset=c["off"]), "fetch_k=1024")


def test_a_caller_stream_and_no_allocation(la, po, small):
    c = small
    keys, counts = _edge_lists(c, 64, 3)
    want = _rerank(la, c["hbm"], c["Q"], keys, counts, 10)
    with HipStreams(la, 1) as st:
        blocks = la.lib().leann_debug_device_blocks()
        for name in ("hbm", "host"):
            got = _rerank(la, c[name], c["Q"], keys, counts, 10, stream=st[0], streams=st)
            assert la.lib().leann_debug_device_blocks() == blocks  # the call allocated nothing
            for x, y in zip(want, got):
                assert x.tobytes() == y.tobytes(), name


# ---- 4. identity on f32 -------------------------------------------------------------------------------------------------------------
def test_identity_on_an_f32_handle(la, po, small):
    """the refined search of an f32 handle over its own rows is its own search at top_k = fetch_k, cut to top_k"""
    c = small
    s = c["s"]
    for fetch_k, top_k, ef in ((20, 10, 48), (33, 33, 40), (10, 1, 10)):
        wk, wd, wc = s.search_batch(c["Q"], fetch_k, ef)
        assert (wc == fetch_k).all()
        for name in ("hbm", "host", "dev"):
            gk, gd, gc = s.search_refined_batch(c["Q"], top_k, fetch_k, ef, c[name])
            assert (gc == top_k).all() and (gk == wk[:, :top_k]).all() and (_bits(gd) == _bits(wd[:, :top_k])).all(), (name, fetch_k)
    ok, od, oc, _ = c["G"].search_batch(c["Q"], 10, 48)
    gk, gd, gc = s.search_refined_batch(c["Q"], 10, 20, 48, c["hbm"])
    assert (gk == ok + np.uint64(c["off"])).all() and (_bits(gd) == _bits(od)).all()


# ---- 5. the point of it: int8 and bf16 walks refined on the exact rows ----------------------------------------------------------------
def _scaled(X):
    """four columns an order of magnitude above the rest, as real embedding models have them"""
    Xs = X.copy()
    Xs[:, [3, 100, 400, 700]] *= 12
    return (Xs / np.linalg.norm(Xs, axis=1, keepdims=True)).astype(np.float32)


class _Case:
    """rows X (scaled columns), one oracle graph, and per narrow type the rows the walk sees (int8: Xq dequantised, bf16: X rounded and
    widened), the oracle over those rows with the same lists, and the narrow handle made from the UNROUNDED X"""

    def __init__(self, la, po, d=768, n=1500):
        self.la, self.po, self.d, self.n = la, po, d, n
        self.X = _scaled(synth(po, n, d))
        self.Q = synth(po, NQ, d, stream=1)
        self.G = po.Graph.build_hnsw(self.X, M=M, efc=EFC)
        self.lists = self.G.export()
        exps, codes = i8_ref.quantize(self.X)
        seen = {"i8": i8_ref.dequantize(codes, exps),
                "bf16": (la.round_bf16(self.X).astype(np.uint32) << 16).view(np.float32)}
        self.seen, self.oracle_graph, self.handle, self._ref = seen, {}, {}, {}
        for name, rt in (("i8", la.RowType.I8), ("bf16", la.RowType.BF16)):
            self.oracle_graph[name] = self.graph_over(seen[name])
            self.handle[name] = self.make(rt)
        self.rows = {p: la.ExactRows.from_host(self.X, placement=p) for p in ("hbm", "host")}

    def graph_over(self, rows):
        lv, uo, a0, aU = self.lists
        return self.po.Graph.from_arrays(rows, M, 2 * M, self.G.max_level, self.G.entry, lv, uo, a0, aU)

    def make(self, row_type, X=None, key_offset=0):
        lv, uo, a0, aU = self.lists
        return self.la.BackendSearcher.from_arrays(self.la.BackendType.Hnsw, self.X if X is None else X, M, 2 * M, self.G.max_level,
                                                   self.G.entry, lv, uo, a0, aU, key_offset=key_offset, row_type=row_type)

    def walk(self, name, k, ef, bm_name=None, bm=None):
        """the oracle's walk over the rows the narrow handle sees, all NQ queries (a smaller batch is its prefix)"""
        key = (name, k, ef, bm_name)
        if key not in self._ref:
            g = self.oracle_graph[name]
            r = g.search_batch(self.Q, k, ef, 0, nthreads=8) if bm is None else g.search_filtered_batch(self.Q, k, ef, bm, 0, nthreads=8)
            self._ref[key] = r
        return self._ref[key]

    def refined(self, name, top_k, fetch_k, ef, bm_name=None, bm=None):
        key = ("refined", name, top_k, fetch_k, ef, bm_name)
        if key not in self._ref:
            wk, _, wc, _ = self.walk(name, fetch_k, ef, bm_name, bm)
            r = refine_ref.rerank(self.po, self.X, self.Q, wk, wc, top_k)
            for a in r:
                a.setflags(write=False)
            self._ref[key] = r
        return self._ref[key]

    def can_tell(self, name):
        """the case tells X from the rows the walk sees: the rows differ, and the walk's distances are not the exact ones"""
        assert (self.X != self.seen[name]).any()
        wk, wd, wc, _ = self.walk(name, 20, 48)
        exact = np.array([self.po.dist_canon(self.Q[q], self.X[int(wk[q, 0])]) for q in range(16)], np.float32)
        assert (_bits(exact) != _bits(wd[:16, 0])).any()

    def close(self):
        for o in list(self.handle.values()) + list(self.rows.values()):
            o.close()


@pytest.fixture(scope="module")
def case(la, po, gpu):
    c = _Case(la, po)
    yield c
    c.close()


def _exact_dists(c, Q, keys, counts):
    out = np.full(keys.shape, np.inf, np.float32)
    for q in range(len(keys)):
        for j in range(int(counts[q])):
            out[q, j] = c.po.dist_canon(Q[q], c.X[int(keys[q, j])])
    return out


@pytest.mark.parametrize("name", ["i8", "bf16"])
def test_narrow_walk_refined_on_exact_rows(la, case, name):
    c = case
    c.can_tell(name)
    top_k, fetch_k, ef = 10, 20, 48
    wk, wd, wc, _ = c.refined(name, top_k, fetch_k, ef)
    uk, ud, _, _ = c.walk(name, top_k, ef)
    assert (wk != uk).any() and (_bits(wd) != _bits(ud)).any()  # refining changes the answer here, so reading the narrow rows would show
    s = c.handle[name]
    for nq in (64, NQ):  # the 16-wave and the 4-wave walk
        for placement in ("hbm", "host"):
            gk, gd, gc = s.search_refined_batch(c.Q[:nq], top_k, fetch_k, ef, c.rows[placement])
            _equal((gk, gd, gc, None), (wk[:nq], wd[:nq], wc[:nq], None), f"{name} nq={nq} {placement}")
    assert (_bits(gd) == _bits(_exact_dists(c, c.Q, gk, gc))).all()  # the f32 value of every returned key, not the narrow rows'
    # the device-pointer form, with the walk's stats
    dQ = la.DeviceArray.from_host(c.Q[:64])
    ok, od = la.DeviceArray((64, top_k), np.uint64), la.DeviceArray((64, top_k), np.float32)
    oc, st = la.DeviceArray(64, np.uint32), la.DeviceArray.from_host(np.zeros((64, 4), np.uint32))
    s.search_refined_batch_device(c.rows["hbm"], dQ.ptr, 64, top_k, fetch_k, ef, ok.ptr, od.ptr, oc.ptr, d_stats=st.ptr)
    _equal((ok.to_host(), od.to_host(), oc.to_host(), None), (wk[:64], wd[:64], wc[:64], None), f"{name} device form")
    ost = c.walk(name, fetch_k, ef)[3][:64]
    assert (st.to_host()[:, :3] == ost).all()
    for a in (dQ, ok, od, oc, st):
        a.free()


@pytest.mark.parametrize("name", ["i8", "bf16"])
def test_narrow_walk_refined_under_a_bitmap(la, case, name):
    c = case
    bm = np.packbits(np.random.default_rng(7).random(c.n) < 0.30, bitorder="little")
    allowed = np.unpackbits(bm, bitorder="little")[: c.n].astype(bool)
    want = c.refined(name, 10, 20, 48, "bm30", bm)
    for nq in (64, NQ):
        gk, gd, gc = c.handle[name].search_refined_batch(c.Q[:nq], 10, 20, 48, c.rows["host"], allow=bm)
        _equal((gk, gd, gc, None), tuple(a[:nq] for a in want[:3]) + (None,), f"{name} bm30 nq={nq}")
        assert (gc == 10).all() and allowed[gk.astype(np.int64)].all()


def test_removed_rows_are_not_returned(la, case):
    c = case
    s = c.make(la.RowType.I8)
    removed = np.random.default_rng(11).random(c.n) < 0.10
    assert s.remove(np.flatnonzero(removed).astype(np.uint64)) == int(removed.sum())
    live = np.packbits(~removed, bitorder="little")
    want = c.refined("i8", 10, 20, 48, "live", live)
    for nq in (64, NQ):
        gk, gd, gc = s.search_refined_batch(c.Q[:nq], 10, 20, 48, c.rows["hbm"])
        _equal((gk, gd, gc, None), tuple(a[:nq] for a in want[:3]) + (None,), f"removed nq={nq}")
        assert not removed[gk[gk != NO_KEY].astype(np.int64)].any()
    s.close()


def test_composite_of_two_int8_shards(la, po, gpu):
    """two int8 shards on one device: the keys are global, the walk's merged lists are refined on rows over all positions"""
    d, n0, n1, top_k, fetch_k, ef = 384, 1024, 768, 10, 20, 48
    X = synth(po, n0 + n1, d)
    X[n0:] *= np.float32(3)
    Q = synth(po, NQ, d, stream=1)
    parts, handles = [], []
    for lo, hi in ((0, n0), (n0, n0 + n1)):
        Xq = i8_ref.dequantized(X[lo:hi])
        G = po.Graph.build_hnsw(Xq, M=M, efc=EFC)
        lv, uo, a0, aU = G.export()
        handles.append(la.BackendSearcher.from_arrays(la.BackendType.Hnsw, X[lo:hi], M, 2 * M, G.max_level, G.entry, lv, uo, a0, aU,
                                                      key_offset=lo, row_type=la.RowType.I8))
        k, dd, cc, _ = G.search_batch(Q, fetch_k, ef, 0, nthreads=8)
        assert (cc == fetch_k).all()
        parts.append((k + np.uint64(lo), dd))
    keys, dists = np.concatenate([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts], axis=1)
    order = np.lexsort((keys, dists), axis=1)[:, :fetch_k]  # by (dist, key): the composite handle's merge
    wk = np.take_along_axis(keys, order, 1)
    want = refine_ref.rerank(po, X, Q, wk, np.full(NQ, fetch_k, np.uint32), top_k)
    s = la.ShardedIndex.from_searchers(handles, take_ownership=True).as_backend()
    rows = la.ExactRows.from_host(X, placement="host")
    for nq in (64, NQ):
        gk, gd, gc = s.search_refined_batch(Q[:nq], top_k, fetch_k, ef, rows)
        _equal((gk, gd, gc, None), tuple(a[:nq] for a in want[:3]) + (None,), f"composite nq={nq}")
    part = la.ExactRows.from_host(X[:n0])  # rows that do not cover the second shard
    with pytest.raises(la.LeannError) as e:
        s.search_refined_batch(Q[:4], top_k, fetch_k, ef, part)
    assert e.value.code == INVALID and "positions" in str(e.value)
    part.close()
    rows.close()
    s.close()


# ---- 6. recall direction --------------------------------------------------------------------------------------------------------------
def test_refining_does_not_lose_recall(po, case):
    """768-d, n = 1 500, scaled columns, M = 8, efc = 48, 704 queries, fetch_k = 40, top_k = 10, ef = 48, against exact f32 truth over X.
    The CPU oracle alone (walk over Xq at k = 40, re-sorted by dist_canon on X) measured, when this test was written: recall@10 of the
    unrefined int8 lists 0.90000, of the refined lists 0.90071.  The GPU equals the oracle bit for bit (the tests above), so
    these are its figures too; the assertion is the direction only."""
    c = case
    truth = po.exact_topk(c.X, c.Q, 10)
    plain, _, _ = c.handle["i8"].search_batch(c.Q, 10, 48)
    refined, _, _ = c.handle["i8"].search_refined_batch(c.Q, 10, 40, 48, c.rows["hbm"])
    r_plain, r_refined = recall_at_k(plain, truth), recall_at_k(refined, truth)
    print(f"recall@10: int8 plain {r_plain:.5f}, refined at fetch_k = 40 {r_refined:.5f}")
    assert r_refined >= r_plain


# ---- 7. refusals with a handle in hand, and nothing left behind -----------------------------------------------------------------------
def test_refusals_and_nothing_left_behind(la, po, gpu):
    L = la.lib()
    n, d = 300, 96
    X, Q = synth(po, n, d), synth(po, 8, d, stream=1)
    G = po.Graph.build_hnsw(X, M=M, efc=EFC)
    lv, uo, a0, aU = G.export()
    la.sync()
    blocks = L.leann_debug_device_blocks()
    s = la.BackendSearcher.from_arrays(la.BackendType.Hnsw, X, M, 2 * M, G.max_level, G.entry, lv, uo, a0, aU, key_offset=1000)
    good = la.ExactRows.from_host(X, key_offset=1000, placement="host")
    wider = la.ExactRows.from_host(np.concatenate([X, X]), key_offset=900)  # covers [900, 1500): fine
    gk, gd, gc = s.search_refined_batch(Q, 5, 10, 32, good)
    hk, hd, hc = s.search_refined_batch(Q, 5, 10, 32, good)
    assert (gc == 5).all() and (gk == hk).all()
    fk, fd, _ = s.search_batch(Q, 10, 32)
    assert (gk == fk[:, :5]).all() and (_bits(gd) == _bits(fd[:, :5])).all()
    wk, _, wc = s.search_refined_batch(Q, 5, 10, 32, wider)  # positions 1000.. are rows 100.. of `wider`: other rows, still answered
    assert (wc == 5).all()
    held = L.leann_debug_device_blocks()
    bad = {
        "dims": la.ExactRows.from_host(X[:, :64].copy(), key_offset=1000),
        "positions": la.ExactRows.from_host(X, key_offset=1001),
        "device": la.ExactRows.from_device(s.device_rows_ptr(), n, d, d, device=1, key_offset=1000),
    }
    short = la.ExactRows.from_host(X[:200], key_offset=1000)
    after_rows = L.leann_debug_device_blocks()
    for word, rows in list(bad.items()) + [("positions", short)]:
        with pytest.raises(la.LeannError) as e:
            s.search_refined_batch(Q, 5, 10, 32, rows)
        assert e.value.code == INVALID and word in str(e.value), (word, str(e.value))
    for top_k, fetch_k, word in ((0, 10, "top_k = 0"), (11, 10, "top_k = 11"), (5, 1025, "fetch_k = 1025")):
        with pytest.raises(la.LeannError) as e:
            s.search_refined_batch(Q, top_k, fetch_k, 32, good)
        assert e.value.code == INVALID and word in str(e.value)
    assert L.leann_debug_device_blocks() == after_rows  # a refused call leaves nothing allocated
    for rows in list(bad.values()) + [short]:
        rows.close()
    assert L.leann_debug_device_blocks() == held
    good.close()
    wider.close()
    s.close()
    assert L.leann_debug_device_blocks() == blocks
