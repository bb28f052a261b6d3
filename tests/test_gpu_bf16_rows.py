"""-m gpu: graph indexes with bf16 rows (include/leann_backend.h "row types", csrc/rows_bf16.hip, csrc/search_bf16.hip).

The definition under test: with r = f32 -> bf16 (round to nearest even) and w = the exact widening, a bf16 index over rows X is the
f32 index over Xr = w(r(X)) with the same graph.  So every comparison here is bit for bit — ids, f32 distance bits, counts,
n_dist_evals, n_hops_base, n_hops_upper — against the oracle walking the same graph on Xr, and the handles are made from the UNROUNDED
X, so that the device rounding kernel is on the path.

Dispatch, as csrc/search_plan.h decides it (family BF16; held to hand-written plans by tests/test_cpu_search_plan.py): T = ceil(ld / 256)
picks the kernel width as for f32 rows; nq <= 512 runs 16 waves per query, larger batches 4, each with its own rows in flight per wave
(ROWS_IN_FLIGHT below); an allow mask picks the filtered kernel; lists of more than 64 ids the wide kernels.

    ld chunks  T    R (4 waves / 16 waves)   d in this file (n)
    1          1    8 / 4                    128 (2000)
    2          2    8 / 4                    260 (2000: partial chunk), 384 (visited set, Vamana)
    3          3    8 / 4                    768 (1500)
    4          4    6 / 4                    900 (1500: partial)
    5 -> 6     6    4 / 3                    1100 (1500: chunk 5 is padding)
    7 -> 8     8    4 / 2                    1600 (1200: chunk 7 is padding)
    9..12      12   2 / 1                    2820 (800: 4 floats in chunk 11)
    13..16     16   2 / - (4 waves always)   3400 (800: T = 14, two padded chunks)

Graphs come from the oracle (po.Graph.build_hnsw / build_vamana, M = 8, efc = 48), as in test_gpu_kernel_matrix.py, so the kernels are
isolated from the GPU builder; test_device_build covers the builder path."""
import ctypes as C
import os

import numpy as np
import pytest

import bf16_ref
from util import recall_at_k, synth

pytestmark = pytest.mark.gpu
EMPTY = 0xFFFFFFFF
NO_KEY = np.iinfo(np.uint64).max
NQ = 704  # > 512: the 4-wave form
M, EFC = 8, 48
WIDTHS = {128: 2000, 260: 2000, 768: 1500, 900: 1500, 1100: 1500, 1600: 1200, 2820: 800, 3400: 800}  # d -> n
ROWS_IN_FLIGHT = {1: (8, 4), 2: (8, 4), 3: (8, 4), 4: (6, 4), 6: (4, 3), 8: (4, 2), 12: (2, 1), 16: (2, None)}  # T -> R of the 4- and the
# 16-wave form (search_plan.h: search_bf16_R4 / _R16); None: that width has no 16-wave form
UNSUPPORTED, INVALID = 5, 1


def _kernel_T(d):
    t = (((d + 3) & ~3) + 255) // 256
    return next(k for k in sorted(ROWS_IN_FLIGHT) if k >= t)


def _from_arrays(la, kind, X, G, deg, deg0, row_type, key_offset=0):
    lv, uo, a0, aU = G.export()
    if kind == 1:
        aU = np.zeros((0, deg), np.uint32)
    return la.BackendSearcher.from_arrays(la.BackendType(kind), X, deg, deg0, G.max_level if kind == 0 else 0, G.entry, lv, uo, a0, aU,
                                          key_offset=key_offset, row_type=row_type)


class _Case:
    """rows X, Xr = w(r(X)), an oracle-built graph whose oracle rows are Xr, and the bf16 handle made from X"""

    def __init__(self, la, po, d, n, kind="hnsw", m=M, nq=NQ):
        self.d, self.n, self.kind, self.po = d, n, kind, po
        self.X = synth(po, n, d)
        self.Xr = bf16_ref.rounded(self.X)
        self.Q = synth(po, nq, d, stream=1)
        if kind == "hnsw":
            self.G, self.algo, self.deg, self.deg0 = po.Graph.build_hnsw(self.Xr, M=m, efc=EFC), 0, m, 2 * m
        else:
            self.G, self.algo, self.deg, self.deg0 = po.Graph.build_vamana(self.Xr, R=24, L=48), 1, 24, 24
        self.s = _from_arrays(la, self.algo, self.X, self.G, self.deg, self.deg0, la.RowType.BF16)
        self.adj0 = np.asarray(self.G.export()[2])
        self._ref = {}

    def oracle(self, nq, k, ef, bm_name=None, bm=None):
        key = (nq, k, ef, bm_name)
        if key not in self._ref:
            if bm is None:
                r = self.G.search_batch(self.Q[:nq], k, ef, self.algo, nthreads=8)
            else:
                r = self.G.search_filtered_batch(self.Q[:nq], k, ef, bm, self.algo, nthreads=8)
            for a in r:
                a.setflags(write=False)
            self._ref[key] = r
        return self._ref[key]

    def can_tell(self):
        """the case distinguishes X from Xr: the rows differ, and so do the oracle's distance bits on the same graph over X"""
        assert (self.X != self.Xr).any()
        lv, uo, a0, aU = self.G.export()
        GX = self.po.Graph.from_arrays(self.X, self.deg, self.deg0, self.G.max_level, self.G.entry, lv, uo, a0, aU)
        _, dx, _, _ = GX.search_batch(self.Q[:16], 10, 48, self.algo, nthreads=8)
        _, dr, _, _ = self.oracle(64, 10, 48)
        assert (dx.view(np.uint32) != dr[:16].view(np.uint32)).any()


@pytest.fixture(scope="module")
def cases(la, po, gpu):
    made = {}

    def get(d, kind="hnsw", m=M, n=None):
        if (d, kind, m) not in made:
            made[d, kind, m] = _Case(la, po, d, n or WIDTHS[d], kind, m)
        return made[d, kind, m]

    yield get
    for c in made.values():
        c.s.close()


def _knob(la, monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, str(value))
    la.lib().leann_debug_reload_env()


def _check(s, Q, ref, what, bm=None):
    """GPU == (keys, dists, counts, stats) of the oracle, bit for bit"""
    ok, od, oc, ost = ref
    s.stats(reset=True)
    gk, gd, gc = s.search_batch(Q, ok.shape[1], what[1]) if bm is None else s.search_filtered_batch(Q, ok.shape[1], what[1], bm)
    st = s.stats()
    assert (gc == oc).all(), what
    assert (gk == ok).all(), f"{what}: ids differ in {(gk != ok).any(axis=1).sum()} of {len(Q)} queries"
    assert (gd.view(np.uint32) == od.view(np.uint32)).all(), what
    assert st["n_dist_evals"] == int(ost[:, 0].sum()), what
    assert st["n_hops_base"] == int(ost[:, 1].sum()), what
    assert st["n_hops_upper"] == int(ost[:, 2].sum()), what
    return gk, gd, gc, st


def _same(c, nq, k, ef, bm_name=None, bm=None):
    return _check(c.s, c.Q[:nq], c.oracle(nq, k, ef, bm_name, bm), (f"d={c.d} nq={nq} k={k} {bm_name or 'plain'}", ef), bm)


def _bitmap(n, frac=0.30, seed=7):
    return np.packbits(np.random.default_rng(seed).random(n) < frac, bitorder="little")


def _legs(c, k=10, ef=48):
    """nq = 64 (16 waves) and 704 (4 waves), plain and under a seeded bitmap allowing about 30 %"""
    bm = _bitmap(c.n)
    for nq in (64, NQ):
        gk, gd, gc, st = _same(c, nq, k, ef)
        assert (gc == k).all() and st["n_hops_base"] > nq  # the oracle fills every answer, and walked
        gk, gd, gc, st = _same(c, nq, k, ef, "bm30", bm)
        assert (gc == k).all() and st["n_hops_base"] > nq
        allowed = np.unpackbits(bm, bitorder="little")[: c.n].astype(bool)
        assert allowed[gk.astype(np.int64)].all()


# ---- 1. kernel matrix ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", list(WIDTHS))
def test_kernel_matrix(la, cases, d):
    c = cases(d)
    assert c.s.row_type() == la.RowType.BF16 and c.s.device_rows_ptr() is None
    c.can_tell()
    T, ld = _kernel_T(d), (d + 3) & ~3
    lens = (c.adj0 != EMPTY).sum(1)
    for nw, r in zip((4, 16), ROWS_IN_FLIGHT[T]):  # a step covers NW x R new rows: a list that leaves a remainder leaves some wave short of R rows
        assert r is None or ((lens > 0) & (lens % (nw * r) != 0)).any(), (d, nw)
    assert (c.Xr[:, 256 * ((ld - 1) // 256):] != 0).any()  # the last chunk that holds data holds some
    _legs(c)
    st = c.s.stats(reset=True)
    gi = c.s.graph_info()
    assert st["algorithmic_bytes"] == st["n_dist_evals"] * d * 2 + st["n_hops_base"] * gi["M0"] * 4 + st["n_hops_upper"] * gi["M"] * 4


def test_vamana_leg(cases):
    c = cases(384, "vamana", n=2000)
    c.can_tell()
    assert ((c.adj0 != EMPTY).sum(1) % (4 * ROWS_IN_FLIGHT[2][0]) != 0).any()
    _legs(c)
    assert c.s.stats()["n_hops_upper"] == 0


# ---- 2. wide lists ------------------------------------------------------------------------------------------------------------------
def test_wide_lists(cases):
    """M = 40: level-0 lists of up to 80 ids take the wide kernels (two list ids per lane of wave 0)"""
    c = cases(768, "hnsw", m=40)
    c.can_tell()
    assert ((c.adj0 != EMPTY).sum(1) > 64).any()
    _legs(c)


# ---- 3. visited set -----------------------------------------------------------------------------------------------------------------
def test_visited_set_moves_to_the_hbm_pool(la, cases, monkeypatch):
    """256 LDS slots: every query outgrows the table (it moves out at 75 % load) and finishes in the HBM pool, in both forms"""
    c = cases(384, "vamana", n=2000)
    _knob(la, monkeypatch, "LEANN_DEBUG_HASH_BITS", 8)
    for nq in (64, NQ):
        ost = c.oracle(nq, 10, 48)[3]
        assert (ost[:, 0] > 256).all()  # more nodes visited than the table has slots: the query must migrate
        gk, gd, gc, st = _same(c, nq, 10, 48)
        assert st["n_table_overflow"] == nq
        bm = _bitmap(c.n)
        _same(c, nq, 10, 48, "bm30", bm)
    _knob(la, monkeypatch, "LEANN_DEBUG_HASH_BITS", None)


# ---- 4. single query ----------------------------------------------------------------------------------------------------------------
def test_single_query_entry_points(cases):
    c = cases(768)
    bm = _bitmap(c.n)
    ok, od, oc, _ = c.oracle(64, 10, 48)
    fk, fd, fc, _ = c.oracle(64, 10, 48, "bm30", bm)
    for q in (0, 5, 63):
        k1, d1 = c.s.search(c.Q[q], 10, 48)
        assert len(k1) == oc[q] and (k1 == ok[q, : oc[q]]).all() and (d1.view(np.uint32) == od[q, : oc[q]].view(np.uint32)).all()
        k2, d2 = c.s.search_filtered(c.Q[q], 10, 48, bm)
        assert len(k2) == fc[q] and (k2 == fk[q, : fc[q]]).all() and (d2.view(np.uint32) == fd[q, : fc[q]].view(np.uint32)).all()


# ---- 5. device build ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,d,deg", [("hnsw", 4000, 768, 16), ("vamana", 3000, 384, 24)])
def test_device_build(la, po, gpu, kind, n, d, deg):
    bt = la.BackendType.Hnsw if kind == "hnsw" else la.BackendType.DiskAnn
    X = synth(po, n, d)
    Xr = bf16_ref.rounded(X)
    Q = synth(po, 96, d, stream=1)
    assert (X != Xr).any()
    dX = la.DeviceArray.from_host(X)
    s = la.BackendSearcher.build_device(bt, dX.ptr, n, d, d, deg, 64, row_type=la.RowType.BF16, may_overwrite=False)
    assert (dX.to_host().view(np.uint32) == X.view(np.uint32)).all()  # may_overwrite = 0: the caller's rows are untouched
    assert s.row_type() == la.RowType.BF16 and s.len() == n
    assert (s.export_rows_bf16() == bf16_ref.round_bf16(X)).all()
    g = s.graph_export(with_vectors=True)
    assert (g["vectors"].view(np.uint32) == Xr.view(np.uint32)).all()
    # the same builder on an uploaded Xr: the same graph (the builder is deterministic)
    dXr = la.DeviceArray.from_host(Xr)
    f = la.BackendSearcher.build_device(bt, dXr.ptr, n, d, d, deg, 64)
    gf = f.graph_export()
    for name in ("levels", "upper_off", "adj0", "adjU", "max_level", "entry", "M", "M0"):
        assert np.array_equal(g[name], gf[name]), name
    algo = 0 if kind == "hnsw" else 1
    G = po.Graph.from_arrays(Xr, g["M"], g["M0"], g["max_level"], g["entry"], g["levels"], g["upper_off"], g["adj0"], g["adjU"])
    ref = G.search_batch(Q, 10, 48, algo, nthreads=8)
    gk, _, _, _ = _check(s, Q, ref, (f"{kind} built on the device", 48))
    assert recall_at_k(gk, po.exact_topk(Xr, Q, 10)) >= 0.9
    fk, fd, fc = f.search_batch(Q, 10, 48)  # ... and the f32 kernels on Xr give the same bits
    assert (fk == gk).all() and (fd.view(np.uint32) == ref[1].view(np.uint32)).all()
    # may_overwrite: the caller's buffer becomes w(r(X)); the same index comes out
    dX2 = la.DeviceArray.from_host(X)
    s2 = la.BackendSearcher.build_device(bt, dX2.ptr, n, d, d, deg, 64, row_type=la.RowType.BF16, may_overwrite=True)
    assert (dX2.to_host().view(np.uint32) == Xr.view(np.uint32)).all()
    g2 = s2.graph_export()
    assert np.array_equal(g2["adj0"], g["adj0"]) and np.array_equal(g2["adjU"], g["adjU"]) and (s2.export_rows_bf16() == bf16_ref.round_bf16(X)).all()
    del dX2  # the handle keeps no f32 rows: the caller's buffer may go
    _check(s2, Q, ref, (f"{kind} built in place", 48))
    # row_type = F32 through the new entry point is the old call
    h = C.c_void_p()
    la._native.check(la.lib().leann_backend_build_device_rows(int(bt), dXr.ptr, n, d, d, deg, 64, 0, 0, int(la.RowType.F32), 0, C.byref(h)))
    f2 = la.BackendSearcher(h, bt)
    assert f2.row_type() == la.RowType.F32 and f2.device_rows_ptr() == dXr.ptr
    g3 = f2.graph_export()
    assert np.array_equal(g3["adj0"], gf["adj0"]) and np.array_equal(g3["adjU"], gf["adjU"]) and np.array_equal(g3["levels"], gf["levels"])
    k3, d3, c3 = f2.search_batch(Q, 10, 48)
    assert (k3 == fk).all() and (d3.view(np.uint32) == fd.view(np.uint32)).all() and (c3 == fc).all()
    for x in (s, s2, f, f2):
        x.close()


# ---- 6. to_rows ---------------------------------------------------------------------------------------------------------------------
def test_to_rows(la, po, gpu):
    n, d = 1500, 768
    X = synth(po, n, d)
    Xr = bf16_ref.rounded(X)
    Q = synth(po, NQ, d, stream=1)
    G = po.Graph.build_hnsw(X, M=M, efc=EFC)  # the graph of the EXACT rows: to_rows keeps it
    f = _from_arrays(la, 0, X, G, M, 2 * M, la.RowType.F32)
    before = f.search_batch(Q, 10, 48)
    b = f.to_rows(la.RowType.BF16)
    assert b.row_type() == la.RowType.BF16 and f.row_type() == la.RowType.F32 and b.len() == n and b.dims() == d
    gb, gf = b.graph_export(with_vectors=True), f.graph_export(with_vectors=True)
    for name in ("levels", "upper_off", "adj0", "adjU", "max_level", "entry", "M", "M0", "n_upper_lists"):
        assert np.array_equal(gb[name], gf[name]), name
    assert (b.export_rows_bf16() == bf16_ref.round_bf16(X)).all()
    assert (gb["vectors"].view(np.uint32) == Xr.view(np.uint32)).all() and (gf["vectors"].view(np.uint32) == X.view(np.uint32)).all()
    lv, uo, a0, aU = G.export()
    Gr = po.Graph.from_arrays(Xr, M, 2 * M, G.max_level, G.entry, lv, uo, a0, aU)
    for nq in (64, NQ):
        _check(b, Q[:nq], Gr.search_batch(Q[:nq], 10, 48, 0, nthreads=8), (f"to_rows nq={nq}", 48))
    after = f.search_batch(Q, 10, 48)  # the source handle still answers as before
    for x, y in zip(before, after):
        assert x.tobytes() == y.tobytes()
    ref = G.search_batch(Q, 10, 48, 0, nthreads=8)
    assert (after[0] == ref[0]).all() and (after[1].view(np.uint32) == ref[1].view(np.uint32)).all()
    assert (ref[1].view(np.uint32) != Gr.search_batch(Q, 10, 48, 0, nthreads=8)[1].view(np.uint32)).any()
    # bf16 -> anything, and a composite handle, are refused
    for rt in (la.RowType.F32, la.RowType.BF16):
        with pytest.raises(la.LeannError) as e:
            b.to_rows(rt)
        assert e.value.code == UNSUPPORTED and "f32 -> bf16" in str(e.value)
    comp = la.ShardedIndex.from_searchers([f], take_ownership=False).as_backend()
    with pytest.raises(la.LeannError) as e:
        comp.to_rows(la.RowType.BF16)
    assert e.value.code == UNSUPPORTED and "leann_sharded_from_handles" in str(e.value)
    comp.close()
    b.close()
    f.close()


# ---- 7. save / open -----------------------------------------------------------------------------------------------------------------
def test_save_open_and_removals(la, cases, tmp_path):
    c = cases(768)
    stem = str(tmp_path / "documents.leann")
    c.s.save(stem)
    gi = c.s.graph_info()
    graph_bytes = c.n + 4 * c.n + 4 * c.n * gi["M0"] + 4 * gi["n_upper_lists"] * gi["M"]
    assert os.path.getsize(tmp_path / "documents.index") == 128 + graph_bytes + c.n * c.d * 2
    raw = (tmp_path / "documents.index").read_bytes()
    assert raw[8:12] == (3).to_bytes(4, "little")
    assert (np.frombuffer(raw[128 + graph_bytes:], np.uint16).reshape(c.n, c.d) == bf16_ref.round_bf16(c.X)).all()
    s = la.HnswSearcher.load(stem, c.d)
    assert s.row_type() == la.RowType.BF16 and s.len() == c.n
    for nq in (64, NQ):
        _check(s, c.Q[:nq], c.oracle(nq, 10, 48), (f"reopened nq={nq}", 48))
    # remove 10 % of the keys: every search runs the filtered walk under the live mask
    rng = np.random.default_rng(11)
    removed = rng.random(c.n) < 0.10
    keys = np.flatnonzero(removed).astype(np.uint64)
    assert s.remove(keys) == len(keys) and s.live_len() == c.n - len(keys)
    live = np.packbits(~removed, bitorder="little")
    bm, pend = s.removed_bitmap()
    assert (np.unpackbits(bm, bitorder="little")[: c.n].astype(bool) == removed).all() and pend > 0
    for nq in (64, NQ):
        gk, _, gc, _ = _check(s, c.Q[:nq], c.oracle(nq, 10, 48, "live", live), (f"after removal nq={nq}", 48))
        assert not removed[gk[gk != NO_KEY].astype(np.int64)].any()
    s.save(stem)
    s.close()
    assert os.path.exists(tmp_path / "documents.tombstones")
    s = la.HnswSearcher.load(stem, c.d)
    assert s.row_type() == la.RowType.BF16 and s.live_len() == c.n - len(keys)
    _check(s, c.Q[:64], c.oracle(64, 10, 48, "live", live), ("removals reopened", 48))
    s.close()


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(la, po, cases, tmp_path):
    c = cases(768)
    L = la.lib()
    Q = c.Q[:64]
    bm = _bitmap(c.n)
    want = c.oracle(64, 10, 48)
    walk = c.oracle(64, 10, 48, "bm30", bm)

    def refused(fn, needle, code=UNSUPPORTED):
        with pytest.raises(la.LeannError) as e:
            fn()
        assert e.value.code == code and needle in str(e.value) and len(str(e.value)) > 20, str(e.value)
        _check(c.s, Q, want, ("after a refusal", 48))  # the handle answers as before

    refused(lambda: c.s.search_filtered_exact_batch(Q, 10, bm), "filtered walk")
    flt = c.s.register_filter(bm)
    refused(lambda: c.s.search_filter_batch(Q, 10, 48, flt, "exact"), "filtered walk")
    for mode in ("auto", "walk"):  # mode 2 picks the walk, whatever the selectivity
        gk, gd, gc = c.s.search_filter_batch(Q, 10, 48, flt, mode)
        assert (gk == walk[0]).all() and (gd.view(np.uint32) == walk[1].view(np.uint32)).all() and (gc == walk[2]).all(), mode
    flt.close()
    tiny = np.zeros((c.n + 7) // 8, np.uint8)
    tiny[:2] = 0xFF  # 16 allowed rows: an f32 index would answer this exactly in mode 2
    flt = c.s.register_filter(tiny)
    gk, gd, gc = c.s.search_filter_batch(Q, 10, 48, flt, "auto")
    tk, td, tc, _ = c.G.search_filtered_batch(Q, 10, 48, tiny, 0, nthreads=8)
    assert (gk == tk).all() and (gd.view(np.uint32) == td.view(np.uint32)).all() and (gc == tc).all()
    flt.close()
    refused(lambda: c.s.consolidate(), "tombstones")
    refused(lambda: c.s.set_row_screen(True), "bf16 rows")
    refused(lambda: c.s.set_row_screen(False), "bf16 rows")
    assert c.s.row_screen_stats() == {"ruled_out": 0, "read_in_full": 0}
    # the file twins: append, remove + repair, sharded open
    stem = str(tmp_path / "documents.leann")
    c.s.save(stem)
    before = (tmp_path / "documents.index").read_bytes()
    b = la.BackendBuilder(la.BackendType.Hnsw)
    refused(lambda: b.add_to_index(c.X[:4], stem, c.d, c.n), "rebuild")
    refused(lambda: b.remove_from_index([1, 2, 3], stem, c.d), "tombstones")
    refused(lambda: la.BackendSearcher.load(la.BackendType.Hnsw, stem, c.d, device="0,0"), "leann_sharded_from_handles")
    assert (tmp_path / "documents.index").read_bytes() == before and not os.path.exists(tmp_path / "documents.tombstones")
    # unknown row types never reach the device
    h = C.c_void_p()
    assert L.leann_backend_to_rows(c.s._h, 7, C.byref(h)) == INVALID and b"row type" in L.leann_last_error() and not h.value
    out = np.zeros(4, np.uint16)
    f = _from_arrays(la, 0, c.Xr[:, :], c.G, c.deg, c.deg0, la.RowType.F32)
    assert L.leann_backend_rows_export_bf16(f._h, out.ctypes.data_as(C.POINTER(C.c_uint16))) == UNSUPPORTED
    f.close()


# ---- 9. composite handles -----------------------------------------------------------------------------------------------------------
def test_composite_of_bf16_shards(la, po, gpu):
    d, n0, n1 = 384, 1024, 768
    X = synth(po, n0 + n1, d)
    Xr = bf16_ref.rounded(X)
    Q = synth(po, NQ, d, stream=1)
    G0, G1 = po.Graph.build_hnsw(Xr[:n0], M=M, efc=EFC), po.Graph.build_hnsw(Xr[n0:], M=M, efc=EFC)
    s0 = _from_arrays(la, 0, X[:n0], G0, M, 2 * M, la.RowType.BF16)
    s1 = _from_arrays(la, 0, X[n0:], G1, M, 2 * M, la.RowType.BF16, key_offset=n0)
    f1 = _from_arrays(la, 0, X[n0:], G1, M, 2 * M, la.RowType.F32, key_offset=n0)
    with pytest.raises(la.LeannError) as e:  # mixing row types
        la.ShardedIndex.from_searchers([s0, f1], take_ownership=False)
    assert e.value.code == INVALID and "row type" in str(e.value)
    f1.close()
    s = la.ShardedIndex.from_searchers([s0, s1], take_ownership=True).as_backend()
    assert s.row_type() == la.RowType.BF16 and s.len() == n0 + n1 and s.n_shards() == 2
    k = 10
    for nq in (64, NQ):
        k0, d0, c0, st0 = G0.search_batch(Q[:nq], k, 48, 0, nthreads=8)
        k1, d1, c1, st1 = G1.search_batch(Q[:nq], k, 48, 0, nthreads=8)
        assert (c0 == k).all() and (c1 == k).all()
        keys = np.concatenate([k0, k1 + np.uint64(n0)], axis=1)
        dists = np.concatenate([d0, d1], axis=1)
        order = np.lexsort((keys, dists), axis=1)[:, :k]  # by (dist, key)
        wk, wd = np.take_along_axis(keys, order, 1), np.take_along_axis(dists, order, 1)
        s.stats(reset=True)
        gk, gd, gc = s.search_batch(Q[:nq], k, 48)
        st = s.stats()
        assert (gc == k).all() and (gk == wk).all() and (gd.view(np.uint32) == wd.view(np.uint32)).all(), nq
        assert st["n_dist_evals"] == int(st0[:, 0].sum() + st1[:, 0].sum()) and st["n_hops_base"] == int(st0[:, 1].sum() + st1[:, 1].sum())
        assert st["n_hops_upper"] == int(st0[:, 2].sum() + st1[:, 2].sum())
        assert st["algorithmic_bytes"] == st["n_dist_evals"] * d * 2 + st["n_hops_base"] * 2 * M * 4 + st["n_hops_upper"] * M * 4
    s.close()


# ---- 10. the device build holds f32 + bf16 rows at its peak, nothing more ---------------------------------------------------------
_NO_PLANES_CHILD = r"""
import sys
import numpy as np
import leann_rs_amd as la
n, d = 1500, 768
X = np.random.default_rng(1).standard_normal((n, d)).astype(np.float32)
X /= np.linalg.norm(X, axis=1, keepdims=True)
dX = la.DeviceArray.from_host(X)
kw = dict(row_type=la.RowType.BF16, may_overwrite=False) if sys.argv[1] == "bf16" else {}
s = la.BackendSearcher.build_device(la.BackendType.Hnsw, dX.ptr, n, d, d, 8, 48, **kw)
print("built", s.row_type().name, s.len())
s.close()
"""


def test_device_build_cuts_no_planes(gpu):
    """LEANN_ROW_SCREEN=1 cuts the split planes — a second full-size copy of the f32 rows — for every f32 handle at any size, and says so
    at LEANN_LOG=info (both are read once per process: hence a child process each).  The f32 build is the control: it logs the cut.
    The bf16 build must not make that copy of rows it is about to drop: its peak is the f32 rows + the bf16 store."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, LEANN_ROW_SCREEN="1", LEANN_LOG="info", PYTHONPATH=root)
    out = {}
    for kind in ("f32", "bf16"):
        r = subprocess.run([sys.executable, "-c", _NO_PLANES_CHILD, kind], capture_output=True, text=True, env=env, cwd=root)
        assert r.returncode == 0, r.stderr
        out[kind] = r
    assert "built F32 1500" in out["f32"].stdout and "split into two planes" in out["f32"].stderr
    assert "built BF16 1500" in out["bf16"].stdout and "split into two planes" not in out["bf16"].stderr, out["bf16"].stderr
