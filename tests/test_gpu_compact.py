"""-m gpu: remove -> consolidate -> COMPACT (include/leann_backend.h "compaction", csrc/compact.hip).

Compaction is a pure renaming, so everything here is exact: the arrays of the result equal tests/compact_ref.py on the consolidated
export bit for bit, and a search of the result returns, through new_to_old, the keys, f32 distance bits, counts and per-query
counters of the same search of the consolidated source.  Rows come from consolidate_ref.random_graph (coordinates in {-2..2}/8: every
distance is exact in f32 in any summation order), so the exact searches can be held to numpy as well.

Shapes: the smallest at which a piece can go wrong — a row pitch that is no multiple of 128 B (d = 40: 160 B), one just past a
multiple (d = 770: 3 088 B), lists of 128 ids, a graph without upper lists, and n = 70 001 (more rows than any tile, grid or scan
block of the kernels covers in one step; the last byte of every bitmap is partly padding)."""
import ctypes as C
import os

import numpy as np
import pytest

import bf16_ref
import compact_ref as cp
import consolidate_ref as cr
from util import SEED

pytestmark = pytest.mark.gpu

EMPTY = cr.EMPTY
NO_KEY = np.iinfo(np.uint64).max
INVALID, UNSUPPORTED = 1, 5
K = 10


def _searcher(la, g, key_offset=0):
    kind = la.BackendType.Hnsw if g["kind"] == "hnsw" else la.BackendType.DiskAnn
    return la.BackendSearcher.from_arrays(kind, g["X"], g["M"], g["M0"], g["max_level"], g["entry"], g["levels"], g["upper_off"],
                                          g["adj0"], g["adjU"], key_offset=key_offset)


def _big_graph(rng, n, d, M, M0, max_level):
    """random_graph's recipe without its O(n^2) sampling: the list of node p on a level names (rank(p) + strictly increasing
    offsets) mod the level's member count — distinct members, never p itself; between W/2 and W ids, EMPTY behind them"""
    X = (rng.integers(-2, 3, (n, d)) / 8.0).astype(np.float32)
    levels = np.minimum(rng.geometric(0.75, n) - 1, max_level).astype(np.uint8)
    levels[int(rng.integers(n))] = max_level
    upper_off = np.zeros(n, np.uint32)
    upper_off[1:] = np.cumsum(levels.astype(np.uint32))[:-1]
    n_upper = int(levels.astype(np.int64).sum())
    adj0 = np.full((n, M0), EMPTY, np.uint32)
    adjU = np.full((n_upper, M), EMPTY, np.uint32)
    for level in range(max_level + 1):
        W = M0 if level == 0 else M
        members = np.flatnonzero(levels >= level)
        m = len(members)
        if m <= W + 1:
            continue
        step = max(1, (m - 1) // W)
        off = np.cumsum(rng.integers(1, step + 1, (m, W)), axis=1)          # 1 <= off < m, strictly increasing
        ids = members[(np.arange(m)[:, None] + off) % m].astype(np.uint32)
        ids[np.arange(W)[None, :] >= rng.integers(W // 2, W + 1, m)[:, None]] = EMPTY
        if level == 0:
            adj0[members] = ids
        else:
            adjU[upper_off[members].astype(np.int64) + level - 1] = ids
    entry = int(np.flatnonzero(levels == levels.max())[0])
    return dict(kind="hnsw", X=X, M=M, M0=M0, max_level=int(levels.max()), entry=entry, levels=levels, upper_off=upper_off, adj0=adj0,
                adjU=adjU)


def removal_pattern(rng, g):
    """about 30 %: a random quarter plus the entry, positions 0 and n - 1, a run of 160 consecutive positions, every second position
    of another stretch and some nodes of level >= 1"""
    n = len(g["X"])
    removed = rng.random(n) < (0.25 if n < 10000 else 0.30)    # (the fixed parts below weigh nothing at a large n)
    removed[[g["entry"], 0, n - 1]] = True
    removed[n // 3: n // 3 + 160] = True
    removed[n // 2: n // 2 + 200: 2] = True
    removed[n // 2 + 1: n // 2 + 200: 2] = False
    removed[np.flatnonzero(g["levels"] >= 1)[:12]] = True
    return removed


#        kind, n, d, M, M0, max_level
CASES = {
    "hnsw_d40_m8": ("hnsw", 2085, 40, 8, 16, 2),          # ld * 4 = 160 B: no multiple of 128
    "hnsw_d770_m4": ("hnsw", 1031, 770, 4, 8, 2),         # pitch 3 088 B
    "hnsw_m64_wide": ("hnsw", 2048, 40, 64, 128, 2),      # lists of 128 ids
    "vamana_r96": ("diskann", 1500, 72, 96, 96, 0),       # no upper lists
    "hnsw_n70001": ("hnsw", 70001, 8, 4, 8, 3),
}


def _graph_dict(s, kind, X=None):
    e = s.graph_export(with_vectors=X is None)
    return dict(kind=kind, X=e["vectors"] if X is None else X, M=e["M"], M0=e["M0"], max_level=e["max_level"], entry=e["entry"],
                levels=e["levels"], upper_off=e["upper_off"], adj0=e["adj0"], adjU=e["adjU"])


class _Case:
    """source handle (removed + consolidated), its export, the compacted handle and its map, the reference's answer"""

    def __init__(self, la, name):
        kind, n, d, M, M0, ml = CASES[name]
        rng = np.random.default_rng(sum(map(ord, name)))
        self.g = _big_graph(rng, n, d, M, M0, ml) if n > 10000 else cr.random_graph(rng, kind, n, d, M, M0, ml)
        self.kind, self.n, self.d = kind, n, d
        self.removed = removal_pattern(rng, self.g)
        if (n - self.removed.sum()) % 8 == 0:                  # the last byte of the result's bitmaps is to be partly padding
            self.removed[np.flatnonzero(~self.removed)[5]] = True
        self.Q =(rng.integers(-2, 3, (700, d)) / 8.0).astype(np.float32)
        self.src = _searcher(la, self.g)
        keys = np.flatnonzero(self.removed).astype(np.uint64)
        assert self.src.remove(keys) == len(keys)
        assert self.src.removed_bitmap()[1] > 0
        self.src.consolidate()
        self.cons = _graph_dict(self.src, kind)
        self.want, self.want_map = cp.compact(self.cons, self.removed)
        self.new, self.map = self.src.compact()
        self.live = n - len(keys)
        self.allow_new = rng.random(self.live) < 0.30


@pytest.fixture(scope="module")
def cases(la, gpu):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Case(la, name)
        return made[name]

    yield get
    for c in made.values():
        c.new.close()
        c.src.close()


def _same_graph(got, want):
    for k in ("M", "M0", "max_level", "entry"):
        assert got[k] == want[k], k
    for k in ("levels", "upper_off", "adj0", "adjU"):
        assert got[k].shape == want[k].shape and (got[k] == want[k]).all(), k
    assert got["X"].shape == want["X"].shape and (got["X"].view(np.uint32) == want["X"].view(np.uint32)).all()


# ---- 1. array-for-array parity -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_arrays_match_the_reference_bit_for_bit(la, cases, name):
    c = cases(name)
    assert c.removed[c.g["entry"]] and c.removed[0] and c.removed[c.n - 1] and 0.25 < c.removed.mean() < 0.45
    assert c.live % 8 != 0                                     # the last byte of the result's bitmaps is partly padding
    assert (c.removed & (c.g["levels"] >= 1)).sum() >= (12 if c.g["max_level"] else 0)
    assert c.map.dtype == np.uint64 and (c.map.astype(np.int64) == c.want_map).all()
    _same_graph(_graph_dict(c.new, c.kind), c.want)
    assert c.new.len() == c.new.live_len() == c.live == c.src.live_len() and c.src.len() == c.n
    bm, pend = c.new.removed_bitmap()
    assert not bm.any() and pend == 0 and len(bm) == (c.live + 7) // 8
    assert c.new.row_type() == c.src.row_type() == la.RowType.F32
    assert type(c.new) is type(c.src)


# ---- 2. searches ---------------------------------------------------------------------------------------------------------------------
def _dev(la, s, Q, k, ef, allow=None, exact=False):
    nq = len(Q)
    dq, dk, dd, dc, ds = la.DeviceArray.from_host(Q), la.DeviceArray((nq, k), np.uint64), la.DeviceArray((nq, k), np.float32), \
        la.DeviceArray(nq, np.uint32), la.DeviceArray((nq, 4), np.uint32)
    da = la.DeviceArray.from_host(allow) if allow is not None else None
    if exact:
        s.search_filtered_exact_batch_device(dq.ptr, nq, k, da.ptr, 0, dk.ptr, dd.ptr, dc.ptr)
    elif allow is not None:
        s.search_filtered_batch_device(dq.ptr, nq, k, ef, da.ptr, 0, dk.ptr, dd.ptr, dc.ptr, ds.ptr)
    else:
        s.search_batch_device(dq.ptr, nq, k, ef, dk.ptr, dd.ptr, dc.ptr, ds.ptr)
    la.sync()
    return dk.to_host(), dd.to_host(), dc.to_host(), (None if exact else ds.to_host()[:, :3])


def _through(keys, counts, new_to_old, new_offset=0):
    """keys of the compacted handle as the source's keys; unfilled slots stay NO_KEY"""
    out = np.full(keys.shape, NO_KEY, np.uint64)
    for i in range(len(keys)):
        out[i, : counts[i]] = new_to_old[(keys[i, : counts[i]] - np.uint64(new_offset)).astype(np.int64)]
        assert (keys[i, counts[i]:] == NO_KEY).all()
    return out


def _same_answers(new, src, new_to_old, what, new_offset=0):
    nk, nd, nc, ns = new
    sk, sd, sc, ss = src
    assert (nc == sc).all(), what
    assert (_through(nk, nc, new_to_old, new_offset) == sk).all(), what
    assert (nd.view(np.uint32) == sd.view(np.uint32)).all(), what
    if ns is not None:
        assert (ns == ss).all(), what


def _exact(X, Q, k, ok_rows):
    ids = np.flatnonzero(ok_rows)
    keys = np.full((len(Q), k), NO_KEY, np.uint64)
    dists = np.full((len(Q), k), np.inf, np.float32)
    counts = np.zeros(len(Q), np.uint32)
    D = (np.float32(1.0) - (Q.astype(np.float64) @ X[ids].astype(np.float64).T).astype(np.float32)).astype(np.float32)
    for i in range(len(Q)):
        o = np.lexsort((ids, D[i]))[:k]
        keys[i, : len(o)], dists[i, : len(o)], counts[i] = ids[o], D[i][o], len(o)
    return keys, dists, counts


@pytest.mark.parametrize("name", list(CASES))
def test_searches_return_the_sources_answers_through_the_map(la, cases, name):
    c = cases(name)
    allow_old = np.zeros(c.n, bool)
    allow_old[c.want_map] = c.allow_new                       # the same bitmap scattered to the old positions
    bm_new, bm_old = np.packbits(c.allow_new, bitorder="little"), np.packbits(allow_old, bitorder="little")
    for nq in (1, 64, 700):
        Q = c.Q[:nq]
        for ef in (10, 48):
            new = _dev(la, c.new, Q, K, ef)
            assert (new[2] > 0).all() and new[3][:, 1].sum() > nq
            _same_answers(new, _dev(la, c.src, Q, K, ef), c.map, (name, nq, ef, "walk"))
        new = _dev(la, c.new, Q, K, 48, allow=bm_new)
        for i in range(nq):
            assert c.allow_new[new[0][i, : new[2][i]].astype(np.int64)].all()
        _same_answers(new, _dev(la, c.src, Q, K, 48, allow=bm_old), c.map, (name, nq, "filtered walk"))
        new = _dev(la, c.new, Q, K, 48, allow=bm_new, exact=True)
        _same_answers(new, _dev(la, c.src, Q, K, 48, allow=bm_old, exact=True), c.map, (name, nq, "exact"))
        if nq <= 64:                                          # and both against numpy's exact top-k over the compacted rows
            ek, ed, ec = _exact(c.want["X"], Q, K, c.allow_new)
            assert (new[2] == ec).all() and (new[0] == ek).all() and (new[1].view(np.uint32) == ed.view(np.uint32)).all()
    # the host-pointer entry points answer as the device ones do
    hk, hd, hc = c.new.search_batch(c.Q[:64], K, 48)
    dk, dd, dc, _ = _dev(la, c.new, c.Q[:64], K, 48)
    assert (hk == dk).all() and (hd.view(np.uint32) == dd.view(np.uint32)).all() and (hc == dc).all()


def test_key_offsets(la, gpu):
    """the new handle returns its own offset + the new position; the map holds the OLD global keys"""
    rng = np.random.default_rng(41)
    n, d, old_off, new_off = 1203, 40, 5000, 777
    g = cr.random_graph(rng, "hnsw", n, d, 8, 16, 2)
    removed = removal_pattern(rng, g)
    Q = (rng.integers(-2, 3, (64, d)) / 8.0).astype(np.float32)
    s = _searcher(la, g, key_offset=old_off)
    s.remove(np.flatnonzero(removed).astype(np.uint64) + np.uint64(old_off))
    s.consolidate()
    live = np.flatnonzero(~removed)
    t, m = s.compact(key_offset=new_off)
    assert (m.astype(np.int64) == live + old_off).all()
    new, src = _dev(la, t, Q, K, 48), _dev(la, s, Q, K, 48)
    for i in range(len(Q)):
        got = new[0][i, : new[2][i]].astype(np.int64)
        assert (got >= new_off).all() and (got < new_off + len(live)).all()
    _same_answers(new, src, m, "key offsets", new_offset=new_off)
    u, m2 = s.compact()                                        # default: the source's own offset
    assert (m2 == m).all()
    keep = _dev(la, u, Q, K, 48)
    assert (keep[0][keep[0] != NO_KEY].astype(np.int64) - old_off == new[0][new[0] != NO_KEY].astype(np.int64) - new_off).all()
    for h in (u, t, s):
        h.close()


# ---- 3. bf16 rows --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [100, 768])                     # store pitch 256 B and 1 536 B
def test_bf16_handle(la, po, gpu, d):
    rng = np.random.default_rng(d)
    n = 1100
    g = cr.random_graph(rng, "hnsw", n, d, 8, 16, 2)
    g["X"] = (g["X"] + rng.integers(-40, 41, (n, d)).astype(np.float32) / np.float32(4096)).astype(np.float32)  # not bf16 numbers
    removed = removal_pattern(rng, g)
    Q = (rng.integers(-2, 3, (704, d)) / 8.0).astype(np.float32)
    f = _searcher(la, g)
    f.remove(np.flatnonzero(removed).astype(np.uint64))
    f.consolidate()
    b = f.to_rows(la.RowType.BF16)
    assert b.row_type() == la.RowType.BF16 and b.live_len() == n - removed.sum() and b.removed_bitmap()[1] == 0
    t, m = b.compact()
    assert t.row_type() == la.RowType.BF16 and t.len() == t.live_len() == len(m) and not t.removed_bitmap()[0].any()
    r = bf16_ref.round_bf16(g["X"])
    assert (bf16_ref.widen(r) != g["X"]).mean() > 0.5          # the rounding matters for these rows
    assert (t.export_rows_bf16() == r[m.astype(np.int64)]).all()
    Xw = bf16_ref.widen(r)
    want, want_map = cp.compact(_graph_dict(b, "hnsw", X=Xw), removed)
    assert (m.astype(np.int64) == want_map).all()
    _same_graph(_graph_dict(t, "hnsw"), want)                  # (the export of a bf16 handle is w(rows))
    G = po.Graph.from_arrays(want["X"], want["M"], want["M0"], want["max_level"], want["entry"], want["levels"], want["upper_off"],
                             want["adj0"], want["adjU"])
    bm = np.packbits(rng.random(len(m)) < 0.30, bitorder="little")
    for nq in (64, 704):
        for ef in (10, 48):
            ok, od, oc, ost = G.search_batch(Q[:nq], K, ef, 0, nthreads=8)
            gk, gd, gc, gs = _dev(la, t, Q[:nq], K, ef)
            assert (gc == oc).all() and (gk == ok).all() and (gd.view(np.uint32) == od.view(np.uint32)).all() and (gs == ost).all()
        ok, od, oc, ost = G.search_filtered_batch(Q[:nq], K, 48, bm, 0, nthreads=8)
        gk, gd, gc, gs = _dev(la, t, Q[:nq], K, 48, allow=bm)
        assert (gc == oc).all() and (gk == ok).all() and (gd.view(np.uint32) == od.view(np.uint32)).all() and (gs == ost).all()
    for h in (t, b, f):
        h.close()


# ---- 4. row screen -------------------------------------------------------------------------------------------------------------------
def test_row_screen_planes_are_cut_for_the_result(la, gpu, monkeypatch):
    monkeypatch.setenv("LEANN_ROW_SCREEN", "1")
    la.lib().leann_debug_reload_env()
    rng = np.random.default_rng(768)
    n, d = 4096, 768
    g = cr.random_graph(rng, "hnsw", n, d, 16, 32, 2)
    removed = removal_pattern(rng, g)
    Q = (rng.integers(-2, 3, (700, d)) / 8.0).astype(np.float32)
    s = _searcher(la, g)
    s.remove(np.flatnonzero(removed).astype(np.uint64))
    s.consolidate()
    t, m = s.compact()
    before = t.row_screen_stats()
    screened = _dev(la, t, Q, K, 48)
    after = t.row_screen_stats()
    assert after["ruled_out"] > before["ruled_out"] and after["ruled_out"] > 0
    t.set_row_screen(False)
    whole = _dev(la, t, Q, K, 48)
    assert t.row_screen_stats()["ruled_out"] in (0, after["ruled_out"])  # nothing more was screened
    assert (screened[0] == whole[0]).all() and (screened[1].view(np.uint32) == whole[1].view(np.uint32)).all()
    assert (screened[2] == whole[2]).all() and (screened[2] == K).all()
    s.set_row_screen(False)
    _same_answers(whole, _dev(la, s, Q, K, 48), m, "screen off against the source")
    t.close()
    s.close()


# ---- 5. the handle is complete: it can lose rows again --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hnsw", "vamana_one_stage"])
def test_remove_and_consolidate_on_the_result(la, gpu, monkeypatch, kind):
    rng = np.random.default_rng(len(kind))
    if kind == "hnsw":
        g = cr.random_graph(rng, "hnsw", 1200, 40, 8, 16, 2)
    else:
        monkeypatch.setenv("LEANN_VAMANA_TWO_STAGE", "0")     # latched when the SOURCE is made ...
        g = cr.random_graph(rng, "diskann", 1024, 128, 32, 32, 0)
    removed = removal_pattern(rng, g)
    s = _searcher(la, g)
    monkeypatch.delenv("LEANN_VAMANA_TWO_STAGE", raising=False)  # ... and carried over by compact, not read again
    s.remove(np.flatnonzero(removed).astype(np.uint64))
    s.consolidate()
    t, m = s.compact()
    k = _graph_dict(t, g["kind"])
    again = rng.random(len(m)) < 0.20
    again[k["entry"]] = True
    assert t.remove(np.flatnonzero(again).astype(np.uint64)) == again.sum() and t.live_len() == len(m) - again.sum()
    assert t.removed_bitmap()[1] == cr.pending(k, again) > 0
    t.consolidate()
    want = cr.consolidate(k, again, alpha=1.2, two_stage=kind == "hnsw")
    assert want["counters"]["repairs"] > 100
    got = t.graph_export()
    assert got["entry"] == want["entry"] and got["max_level"] == want["max_level"] and not again[got["entry"]]
    assert (got["adj0"] == want["adj0"]).all() and (got["adjU"] == want["adjU"]).all()
    u, m2 = t.compact()                                        # and be compacted again
    assert (m2.astype(np.int64) == np.flatnonzero(~again)).all() and u.len() == len(m2)
    for h in (u, t, s):
        h.close()


# ---- 6. files ------------------------------------------------------------------------------------------------------------------------
def test_files(la, gpu, tmp_path):
    rng = np.random.default_rng(6)
    n, d = 1037, 40
    g = cr.random_graph(rng, "hnsw", n, d, 8, 16, 2)
    removed = removal_pattern(rng, g)
    keys = np.flatnonzero(removed).astype(np.uint64)
    Q = (rng.integers(-2, 3, (64, d)) / 8.0).astype(np.float32)
    hn = la.BackendType.Hnsw
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    (tmp_path / "c").mkdir()
    stem_a, stem_b, stem_c = (str(tmp_path / x / "documents.leann") for x in "abc")
    file_a, file_b, file_c = (str(tmp_path / x / "documents.index") for x in "abc")
    side_a, side_b = (str(tmp_path / x / "documents.tombstones") for x in "ab")
    # b: removals pending consolidation, saved with their sidecar
    s = _searcher(la, g)
    s.remove(keys)
    s.save(stem_b)
    assert os.path.exists(side_b)
    s.consolidate()
    # a: the handle route, saved over a stale sidecar
    s.save(stem_a)
    assert os.path.exists(side_a)
    t, m = s.compact()
    t.save(stem_a)
    assert not os.path.exists(side_a)
    want = t.search_batch(Q, K, 48)
    # c: an index of `live` rows that never lost any
    fresh = _searcher(la, cp.compact(_graph_dict(s, "hnsw"), removed)[0])
    fresh.save(stem_c)
    assert os.path.getsize(file_a) == os.path.getsize(file_c) < os.path.getsize(file_b)
    for h in (fresh, t, s):
        h.close()
    o = la.BackendSearcher.load(hn, stem_a, d)
    assert o.len() == o.live_len() == len(m) and not o.removed_bitmap()[0].any()
    got = o.search_batch(Q, K, 48)
    assert (got[0] == want[0]).all() and (got[1].view(np.uint32) == want[1].view(np.uint32)).all() and (got[2] == want[2]).all()
    o.close()
    # the file twin on b: a map without room is refused and nothing is written ...
    bytes_b, bytes_side = open(file_b, "rb").read(), open(side_b, "rb").read()
    small = np.zeros(len(m), np.uint64)
    live = C.c_size_t(0)
    rc = la.lib().leann_backend_compact_index(int(hn), d, os.fsencode(stem_b), small.ctypes.data_as(la._native.u64p), len(m) - 1, C.byref(live))
    assert rc == INVALID and str(len(m)) in la.lib().leann_last_error().decode() and live.value == len(m)
    assert open(file_b, "rb").read() == bytes_b and open(side_b, "rb").read() == bytes_side
    # ... then: the same file bytes and the same map as the handle route
    m_b = la.BackendBuilder(hn).compact_index(stem_b, d)
    assert (m_b == m).all() and not os.path.exists(side_b)
    assert open(file_b, "rb").read() == open(file_a, "rb").read()
    # nothing removed: the identity, and the file is not touched
    before = open(file_c, "rb").read()
    stamp = os.stat(file_c).st_mtime_ns
    m_c = la.BackendBuilder(hn).compact_index(stem_c, d)
    assert (m_c == np.arange(len(m), dtype=np.uint64)).all()
    assert open(file_c, "rb").read() == before and os.stat(file_c).st_mtime_ns == stamp


# ---- 7. refusals and leaks -------------------------------------------------------------------------------------------------------------
def _refused(la, s, code, needle):
    h = C.c_void_p(0x1)
    m = np.zeros(max(s.len(), 1), np.uint64)
    rc = la.lib().leann_backend_compact(s._h, 0, C.byref(h), m.ctypes.data_as(la._native.u64p))
    msg = la.lib().leann_last_error().decode()
    assert rc == code and needle in msg, (rc, msg)
    assert not h.value                                         # no handle made


def test_refusals_leave_the_source_as_it_was_and_nothing_behind(la, po, gpu):
    blocks = la.lib().leann_debug_device_blocks
    rng = np.random.default_rng(7)
    n, d = 1029, 40
    g = cr.random_graph(rng, "hnsw", n, d, 8, 16, 2)
    removed = removal_pattern(rng, g)
    Q = (rng.integers(-2, 3, (64, d)) / 8.0).astype(np.float32)
    start = blocks()
    s = _searcher(la, g)
    s.remove(np.flatnonzero(removed).astype(np.uint64))
    s.search_batch(Q, K, 48)                                   # (the handle's own search scratch exists from here on)
    answers = s.search_batch(Q, K, 48)
    held = blocks()
    # live lists still name removed positions
    assert s.removed_bitmap()[1] > 0
    _refused(la, s, INVALID, "leann_backend_consolidate")
    assert blocks() == held
    got = s.search_batch(Q, K, 48)
    assert all((a == b).all() for a, b in zip(got, answers))
    # null arguments
    assert la.lib().leann_backend_compact(None, 0, C.byref(C.c_void_p()), None) == INVALID
    assert la.lib().leann_backend_compact(s._h, 0, None, None) == INVALID and "null" in la.lib().leann_last_error().decode()
    # a composite handle
    a, b = _searcher(la, g), _searcher(la, g, key_offset=n)
    comp = la.ShardedIndex.from_searchers([a, b], take_ownership=True).as_backend()
    _refused(la, comp, UNSUPPORTED, "leann_sharded_from_handles")
    comp.close()
    # a recompute-on handle
    Lc, chk = la.lib(), la._native.check
    F, W = po.synth_features(SEED, 64, 64, 1.0, 0, 0, 600), po.synth_weights(SEED, 64, 64)
    dF, dW = la.DeviceArray.from_host(F), la.DeviceArray.from_host(W)
    r, hb = C.c_void_p(), C.c_void_p()
    chk(Lc.leann_recompute_create(dF.ptr, 600, 64, dW.ptr, 64, 0, 0, C.byref(r)))
    chk(Lc.leann_recompute_build_index(r, 0, 8, 64, C.byref(hb)))
    feat = la.BackendSearcher(hb, la.BackendType.Hnsw)
    assert feat.row_type() == la.RowType.Features
    _refused(la, feat, UNSUPPORTED, "cannot consolidate")
    feat.close()
    Lc.leann_recompute_close(r)
    del dF, dW
    assert blocks() == held
    # nothing live
    e = _searcher(la, g)
    e.remove(np.arange(n, dtype=np.uint64))
    e.consolidate()
    assert e.removed_bitmap()[1] == 0 and e.live_len() == 0
    _refused(la, e, INVALID, "nothing is live")
    e.close()
    assert blocks() == held
    # the full round trip
    s.consolidate()
    answers = s.search_batch(Q, K, 48)
    held = blocks()
    t, m = s.compact()
    assert blocks() > held
    got = t.search_batch(Q, K, 48)
    assert (got[2] == answers[2]).all() and (_through(got[0], got[2], m) == answers[0]).all()
    t.close()
    assert blocks() == held
    got = s.search_batch(Q, K, 48)
    assert all((x == y).all() for x, y in zip(got, answers))
    p, mp = _searcher(la, g), None                             # nothing removed: a plain copy, the identity map
    held_p = blocks()
    c, mp = p.compact()
    assert (mp == np.arange(n, dtype=np.uint64)).all() and c.len() == n
    _same_graph(_graph_dict(c, "hnsw"), {**g})
    c.close()
    assert blocks() == held_p
    p.close()
    s.close()
    assert blocks() == start
