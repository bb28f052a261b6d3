"""-m gpu: every narrow beam-search kernel api.hip can launch, against the oracle walk, bit for bit.

Dispatch, as csrc/search_plan.h decides it (its rules are held to hand-written plans by tests/test_cpu_search_plan.py).  Stored f32 rows:
T = ceil(ld / 256) picks <T, R> (R rows in flight per wave); the batch picks NW = 16 (nq <= 384), 8 (<= 640) or 4 waves per query
(LEANN_DEBUG_NW overrides); an allow mask picks the filtered kernel.  "nat" = test_natural_dispatch, "nw" = test_forced_wave_counts,
"filt" = test_filtered, "vam" = test_diskann_leg, each parametrised by the row width d.

    ld chunks  kernel <T, R>   d in this file             beam_search_kernel<T,R,NW,false>          beam_search_filtered_kernel<T,R,NW>
    1          <1, 4>          128                        NW 16 / 8 / 4: nat[128] 64/512/704, nw    NW 16 / 8 / 4: filt[128] 64/512/704
    2          <2, 4>          384, 260 (partial)         nat, nw, vam[384]                         filt[384], filt[260]
    3          <3, 4>          768                        nat, nw                                   filt[768]
    4          <4, 3>          1024, 900 (partial)        nat, nw, vam[1024]                        filt[1024], filt[900]
    5 -> 6     <6, 2>          1100 (chunk 5 is padding)  nat, nw                                   filt[1100]
    6          <6, 2>          1536                       nat, nw                                   filt[1536]
    7 -> 8     <8, 2>          1600 (chunk 7 is padding)  nat, nw                                   filt[1600]
    8          <8, 2>          2048                       nat, nw                                   filt[2048]
    9..12      <12, 1>         2820 (4 floats in chunk 11) nat, nw                                  filt[2820]
    13..16     <16, 1>         3400 (T = 14: two padded)  nat, nw                                   filt[3400]

  * hash_bits: 12 (4096 slots) when ld <= 512 and ef <= 64, else pick(ef) = 13 here: test_small_visited_table (d = 384,
    ef 64 / 65; LEANN_DEBUG_HASH_BITS=8 moves every query to the HBM pool inside the <2, 4, 16> and <2, 4, 4> kernels).
  * batch thresholds 384 | 385 and 640 | 641: test_batch_size_thresholds (d = 128).
  * beam_search_kernel<T,R,NW,true> (BUILD: the query is a stored row, SearchArgs::q_rows): launched by the on-device builder only
    (build.hip), with the wave count its batch sizes pick; no searcher entry point sets q_rows and its beams are not returned, so
    there is no oracle to hold it to bit for bit.  T = 1, 3, 6: test_gpu_builder_quality.py and the GPU-built fixtures of
    test_gpu_row_screen.py (d = 520 .. 1536); every other width: test_built_on_device_at_the_widths_no_other_test_builds, by the
    builder's bars (valid lists, search == oracle on the export, recall).  wide_beam_search_kernel<..,true>: test_gpu_wide_degree.py.
  * wide_beam_search_kernel / wide_beam_search_filtered_kernel <T,R,16|4> (lists of more than 64 ids): test_gpu_wide_degree.py.
  * beam_search_screen_kernel<3, 4> / <6, 2> (split planes, 4-wave unfiltered batches): test_gpu_row_screen.py, whose fixture dims
    520, 700, 768 run <3, 4> and 1100, 1280 (T = 5 in the 6-kernel), 1536 run <6, 2>.
    test_gpu_row_screen_wide.py: <3, 4> over lists of 64 (M = 32).  test_gpu_row_screen_edges.py: 516 (<3, 4>) and 1028 (<6, 2>, the
    sixth chunk wholly past the plane row) — plane rows ending in a 64-element tail —, <6, 2> over lists of 64 (1100, M = 32), Vamana
    handles (R = 32 / 64 at 768, R = 32 at 1100), LEANN_DEBUG_HASH_BITS=8 (every query moves to the HBM pool inside <3, 4> and <6, 2>),
    nq = 641 | 640 | 384 on one handle, k = ef = 1, rows x 37.5 / queries x 1e-3 and rows x 1e-30 / queries x 1e-10, rows holding an
    infinity, a two-shard composite handle.  All three files hold the device's ruled-out count to the oracle's counting search.

Recompute-on graphs (bf16 feature rows, family FEAT / FEAT256 of search_plan.h; 16 waves for nq <= 512, else 4; "rc" = test_recompute_on_wide_features):

    feat_h      kernel                                             case
    <= 256      beam_search_feat[_filtered]_kernel<1, R1, 16|4>    rc[100] (row_bytes 208, inline norm), nq 64 / 704, plain + bitmap
    == 256      beam_search_feat256[_filtered]_kernel<1,16>/<G,4>  test_gpu_recompute.py, test_gpu_filtered.py (h = 256)
    257..512    beam_search_feat[_filtered]_kernel<2, 6, 16|4>     rc[300], rc[448], rc[496], nq 64 / 704, plain + bitmap
    513..1024   beam_search_feat[_filtered]_kernel<4, 4, 16|4>     NOT reachable through leann_recompute_create at any dims: the widest
                                                                   accepted h is 496 (WIDEST_H below).  A version-2 index file may hold
                                                                   feat_h <= 1024 (indexfile.hip: load_own_file), so
                                                                   test_v2_file_with_640_features opens a hand-written one (T = 3 in the
                                                                   4-kernel: a whole padded chunk), nq 64 / 704, plain + bitmap
    any         wide_beam_search_feat*                             test_gpu_wide_degree.py::test_recompute_on_graph_of_degree_64

Graphs come from the oracle (po.Graph.build_hnsw / build_vamana) and reach the device through BackendSearcher.from_arrays, so the
kernels are isolated from the GPU builder.  Every comparison: ids, f32 distance bits, counts, n_dist_evals, n_hops_base, n_hops_upper.
Every case also shows, on the oracle's own numbers, that it walked something: full answers, more base hops than queries, a list whose
length leaves a remainder for the form's NW x R rows per step, and a non-zero value in the last partial chunk."""
import ctypes as C

import numpy as np
import pytest

from util import SEED, recall_at_k, synth, write_gx2

pytestmark = pytest.mark.gpu
EMPTY = 0xFFFFFFFF
NQ = 704  # > 640: the 4-wave form
M, EFC = 8, 48
WIDTHS = {128: 2000, 384: 2000, 260: 2000, 768: 1500, 1024: 1500, 900: 1500, 1100: 1500, 1536: 1200, 2048: 1200, 1600: 1200,
          2820: 800, 3400: 800}  # d -> n
PADDED_CHUNKS = {1100: 1, 1600: 1, 3400: 2}  # T = 5 in the 6-kernel, 7 in the 8-kernel, 14 in the 16-kernel
ROWS_IN_FLIGHT = {1: 4, 2: 4, 3: 4, 4: 3, 6: 2, 8: 2, 12: 1, 16: 1}  # R by T of the stored-f32 kernels (search_plan.h: search_f32_R)


def _kernel_T(d):
    t = (((d + 3) & ~3) + 255) // 256
    return next(k for k in sorted(ROWS_IN_FLIGHT) if k >= t)


class _Case:
    def __init__(self, la, po, d, n, kind="hnsw"):
        self.d, self.n, self.kind = d, n, kind
        self.X = synth(po, n, d)
        self.Q = synth(po, NQ, d, stream=1)
        if kind == "hnsw":
            self.G, self.algo = po.Graph.build_hnsw(self.X, M=M, efc=EFC), 0
            lv, uo, a0, aU = self.G.export()
            self.s = la.BackendSearcher.from_arrays(la.BackendType.Hnsw, self.X, M, 2 * M, self.G.max_level, self.G.entry, lv, uo, a0, aU)
        else:  # the oracle's sorted-list GreedySearch over a Vamana graph
            R = 24
            self.G, self.algo = po.Graph.build_vamana(self.X, R=R, L=48), 1
            lv, uo, a0, aU = self.G.export()
            self.s = la.BackendSearcher.from_arrays(la.BackendType.DiskAnn, self.X, R, R, 0, self.G.entry, lv, uo, a0, np.zeros((0, R), np.uint32))
        self.adj0 = np.asarray(a0)
        self._ref = {}

    def oracle(self, nq, k, ef, bm_name=None, bm=None):
        """the oracle's answer for the first nq queries: computed once, shared by the tests that need it"""
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


@pytest.fixture(scope="module")
def cases(la, po, gpu):
    made = {}

    def get(d, kind="hnsw"):
        if (d, kind) not in made:
            made[d, kind] = _Case(la, po, d, WIDTHS[d], kind)
        return made[d, kind]

    yield get
    for c in made.values():
        c.s.close()


def _knob(la, monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, str(value))
    la.lib().leann_debug_reload_env()


def _same(c, nq, k, ef, bm_name=None, bm=None):
    """GPU == oracle on the first nq queries of the case, bit for bit; returns (GPU keys, dists, counts, the handle's stats, oracle stats)"""
    ok, od, oc, ost = c.oracle(nq, k, ef, bm_name, bm)
    c.s.stats(reset=True)
    if bm is None:
        gk, gd, gc = c.s.search_batch(c.Q[:nq], k, ef)
    else:
        gk, gd, gc = c.s.search_filtered_batch(c.Q[:nq], k, ef, bm)
    st = c.s.stats()
    what = f"d={c.d} nq={nq} k={k} ef={ef} {bm_name or 'plain'}"
    assert (gc == oc).all(), what
    assert (gk == ok).all(), f"{what}: ids differ in {(gk != ok).any(axis=1).sum()} of {nq} queries"
    assert (gd.view(np.uint32) == od.view(np.uint32)).all(), what
    assert st["n_dist_evals"] == int(ost[:, 0].sum()), what
    assert st["n_hops_base"] == int(ost[:, 1].sum()), what
    assert st["n_hops_upper"] == int(ost[:, 2].sum()), what
    return gk, gd, gc, st, ost


def _bitmaps(c):
    """a shared bitmap at 10 % and one bitmap per query at 20 %"""
    rng = np.random.default_rng(7)
    shared = np.packbits(rng.random(c.n) < 0.10, bitorder="little")
    per_query = np.packbits(rng.random((NQ, c.n)) < 0.20, axis=-1, bitorder="little")
    return shared, per_query


# ---- 1. stored f32 rows: T x waves x filter ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", list(WIDTHS))
def test_case_reaches_the_remainder_and_the_padding(cases, d):
    """what the other tests of a width rely on, from the exported graph and the rows alone"""
    c = cases(d)
    T, ld = _kernel_T(d), (d + 3) & ~3
    lens = (c.adj0 != EMPTY).sum(1)
    for nw in (4, 8, 16):  # a step covers NW x R new rows, wave w takes rows w, w + NW, ...: a shorter list leaves some wave nrows < R
        assert ((lens > 0) & (lens % (nw * ROWS_IN_FLIGHT[T]) != 0)).any(), (d, nw)
    last = 256 * ((ld - 1) // 256)  # first element of the last chunk that holds data
    assert (c.X[:, last:] != 0).any()
    assert T - (ld + 255) // 256 == PADDED_CHUNKS.get(d, 0)  # whole chunks of the kernel past the row: every lane must read zeros


@pytest.mark.parametrize("d", list(WIDTHS))
def test_natural_dispatch(cases, d):
    """batches of 64 (16 waves), 512 (8 waves) and 704 (4 waves) through the form the batch size picks"""
    c = cases(d)
    for nq in (64, 512, NQ):
        for k, ef in ((10, 48), (1, 1)):
            gk, gd, gc, st, ost = _same(c, nq, k, ef)
            assert (gc == k).all()
            if ef == 48:
                assert st["n_hops_base"] > nq and int(ost[:, 1].sum()) > nq


@pytest.mark.parametrize("d", list(WIDTHS))
def test_forced_wave_counts(la, cases, monkeypatch, d):
    """every wave count on the same 96 queries"""
    c = cases(d)
    for nw in (4, 8, 16):
        _knob(la, monkeypatch, "LEANN_DEBUG_NW", nw)
        gk, gd, gc, st, ost = _same(c, 96, 10, 40)
        assert (gc == 10).all() and st["n_hops_base"] > 96
    _knob(la, monkeypatch, "LEANN_DEBUG_NW", None)


@pytest.mark.parametrize("d", list(WIDTHS))
def test_filtered(cases, d):
    """the filtered kernels: 16 waves (64 queries), 8 (512) and 4 (704), a shared bitmap and one bitmap per query"""
    c = cases(d)
    shared, per_query = _bitmaps(c)
    allowed = np.unpackbits(shared, bitorder="little")[: c.n].astype(bool)
    for nq in (64, 512, NQ):
        gk, gd, gc, st, ost = _same(c, nq, 10, 48, "shared", shared)
        assert (gc >= 1).all()  # every query finds an allowed row
        assert allowed[gk[gk != np.iinfo(np.uint64).max].astype(np.int64)].all()
        assert st["n_hops_base"] > nq
    for nq in (64, NQ):
        _same(c, nq, 10, 48, f"per_query{nq}", per_query[:nq])


@pytest.mark.parametrize("d", [384, 1024])
def test_diskann_leg(cases, d):
    c = cases(d, "vamana")
    lens = (c.adj0 != EMPTY).sum(1)
    assert (lens % (4 * ROWS_IN_FLIGHT[_kernel_T(d)]) != 0).any()
    for nq in (64, NQ):
        gk, gd, gc, st, ost = _same(c, nq, 10, 48)
        assert (gc == 10).all() and st["n_hops_base"] > nq and st["n_hops_upper"] == 0


def _valid_lists(adj0, n):
    a0 = np.asarray(adj0)
    valid = a0 != EMPTY
    assert (valid[:, :-1] >= valid[:, 1:]).all() and (a0[valid] < n).all()  # compact lists of row ids
    assert not (a0 == np.arange(n, dtype=np.uint32)[:, None]).any()         # no self-edges
    srt = np.sort(np.where(valid, a0, EMPTY).astype(np.int64), axis=1)
    assert not ((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] != EMPTY)).any()   # no duplicate ids


@pytest.mark.parametrize("d", [384, 1024, 1100, 1600, 2048, 2820, 3400])
def test_built_on_device_at_the_widths_no_other_test_builds(la, po, cases, d):
    """beam_search_kernel<T, R, NW, true>, the construction search, at T = 2, 4, 5 -> 6, 7 -> 8, 8, 12 and 14 -> 16.  What it returns
    is seen only through the graph the builder makes of it, so the bars are the builder's: valid lists, the walk over the built graph
    equal to the oracle's walk over its export, and recall@10 >= 0.9 against exact search — the bar smoke() sets for build + search."""
    c = cases(d)
    dX = la.DeviceArray.from_host(c.X)
    s = la.BackendSearcher.build_device(la.BackendType.Hnsw, dX.ptr, c.n, d, d, M, EFC)
    g = s.graph_export()
    assert g["M"] == M and g["M0"] == 2 * M
    _valid_lists(g["adj0"], c.n)
    G = po.Graph.from_arrays(c.X, M, 2 * M, g["max_level"], g["entry"], g["levels"], g["upper_off"], g["adj0"], g["adjU"])
    ok, od, oc, ost = G.search_batch(c.Q, 10, 48, 0, nthreads=8)
    s.stats(reset=True)
    gk, gd, gc = s.search_batch(c.Q, 10, 48)
    st = s.stats()
    assert (gc == oc).all() and (gk == ok).all() and (gd.view(np.uint32) == od.view(np.uint32)).all()
    assert st["n_dist_evals"] == int(ost[:, 0].sum()) and st["n_hops_base"] == int(ost[:, 1].sum())
    assert recall_at_k(gk, po.exact_topk(c.X, c.Q, 10)) >= 0.9
    s.close()


# ---- 2. dispatch boundaries and the small visited table ------------------------------------------------------------------------------
def test_batch_size_thresholds(la, po, gpu):
    """384 | 385 queries: 16 -> 8 waves; 640 | 641: 8 -> 4.  Each batch equals the oracle, and a query's row is the same in every batch."""
    n, d, m = 3000, 128, 16
    X = synth(po, n, d)
    Q = synth(po, 641, d, stream=1)
    G = po.Graph.build_hnsw(X, M=m, efc=64)
    lv, uo, a0, aU = G.export()
    s = la.BackendSearcher.from_arrays(la.BackendType.Hnsw, X, m, 2 * m, G.max_level, G.entry, lv, uo, a0, aU)
    ok, od, oc, ost = G.search_batch(Q, 10, 64, 0, nthreads=8)
    assert (oc == 10).all()
    got = {}
    for nq in (384, 385, 640, 641):
        s.stats(reset=True)
        gk, gd, gc = got[nq] = s.search_batch(Q[:nq], 10, 64)
        st = s.stats()
        assert (gc == oc[:nq]).all() and (gk == ok[:nq]).all() and (gd.view(np.uint32) == od[:nq].view(np.uint32)).all(), nq
        assert st["n_dist_evals"] == int(ost[:nq, 0].sum()) and st["n_hops_base"] == int(ost[:nq, 1].sum()), nq
        assert st["n_hops_upper"] == int(ost[:nq, 2].sum()), nq
    for a, b in ((384, 385), (385, 640), (640, 641), (384, 641)):
        for x, y in zip(got[a], got[b]):  # keys, dists, counts
            assert x[:a].tobytes() == y[:a].tobytes(), (a, b)
    s.close()


def test_small_visited_table(la, cases, monkeypatch):
    """ld <= 512: ef = 64 takes the 4096-slot table, ef = 65 the 8192-slot one; with 256 slots forced, queries outgrow LDS and move
    to the HBM pool inside the T = 2 kernels (16 waves at 64 queries, 4 waves at 704)."""
    c = cases(384)
    for ef in (64, 65):
        for nq in (64, NQ):
            gk, gd, gc, st, ost = _same(c, nq, 10, ef)
            print(f"d=384 ef={ef} nq={nq}: n_table_overflow {st['n_table_overflow']}")
            assert (gc == 10).all()
    _knob(la, monkeypatch, "LEANN_DEBUG_HASH_BITS", 8)
    for ef in (64, 65):
        for nq in (64, NQ):
            gk, gd, gc, st, ost = _same(c, nq, 10, ef)
            print(f"d=384 ef={ef} nq={nq}, 256 slots: n_table_overflow {st['n_table_overflow']}")
            # 256 slots cannot hold more than 256 visited nodes (the kernel moves out at 75 % load, sooner)
            must = int((ost[:, 0] > 256).sum())
            assert must > 0 and st["n_table_overflow"] >= must
    _knob(la, monkeypatch, "LEANN_DEBUG_HASH_BITS", None)


class _WanderingCase(_Case):
    """i.i.d. rows (searches wander) under an oracle-built HNSW graph; the handle `s` is made by the test, after its knobs are set"""

    def __init__(self, po, n, d, m):
        self.d, self.n, self.algo, self._ref = d, n, 0, {}
        self.X = synth(po, n, d, r=0)
        self.Q = synth(po, NQ, d, stream=1, r=0)
        self.G = po.Graph.build_hnsw(self.X, M=m, efc=64)


def test_visited_set_climbs_both_pools_in_both_loop_forms(la, po, gpu, monkeypatch):
    """The visited-set migration (csrc/hop_migrate.cuh), both branches — LDS -> pool 1, then pool 1 -> pool 2, which copies from an
    HBM table, releases the old table's lock and keeps the generation — in both forms of the hop loop (64 queries: 16 waves; 704: 4
    waves), plain and under a shared 10 % bitmap.  A 256-slot LDS table and 1024-slot pool-1 tables over 5000 i.i.d. rows: the
    index does not fit a pool-1 table, so the handle gets a pool 2, and every query evaluates more nodes than pool 1 has slots."""
    n, d, m, k, ef = 5000, 128, 16, 10, 400
    c = _WanderingCase(po, n, d, m)
    bm = np.packbits(np.random.default_rng(7).random(n) < 0.10, bitorder="little")
    legs = [(nq, name, mask) for nq in (64, NQ) for name, mask in ((None, None), ("shared", bm))]
    for nq, name, mask in legs:  # on the oracle's own numbers, before the GPU is touched: no leg can pass without reaching pool 2
        ok, od, oc, ost = c.oracle(nq, k, ef, name, mask)
        assert int(ost[:, 0].min()) > 1024, (nq, name, int(ost[:, 0].min()))
    _knob(la, monkeypatch, "LEANN_DEBUG_HASH_BITS", 8)    # LDS table: 256 slots
    _knob(la, monkeypatch, "LEANN_DEBUG_GPOOL_BITS", 10)  # pool 1: 1024 slots (the pools are sized at a handle's first use)
    lv, uo, a0, aU = c.G.export()
    c.s = la.BackendSearcher.from_arrays(la.BackendType.Hnsw, c.X, m, 2 * m, c.G.max_level, c.G.entry, lv, uo, a0, aU)
    dQ, dbm = la.DeviceArray.from_host(c.Q), la.DeviceArray.from_host(bm)
    try:
        for nq, name, mask in legs:
            gk, gd, gc, st, ost = _same(c, nq, k, ef, name, mask)
            dk, dd, dc = la.DeviceArray((nq, k), np.uint64), la.DeviceArray((nq, k), np.float32), la.DeviceArray(nq, np.uint32)
            dst = la.DeviceArray.from_host(np.full((nq, 4), 0xABCD1234, np.uint32))
            if mask is None:
                c.s.search_batch_device(dQ.ptr, nq, k, ef, dk.ptr, dd.ptr, dc.ptr, d_stats=dst.ptr)
            else:
                c.s.search_filtered_batch_device(dQ.ptr, nq, k, ef, dbm.ptr, 0, dk.ptr, dd.ptr, dc.ptr, d_stats=dst.ptr)
            la.sync()
            per_query = dst.to_host()
            what = f"nq={nq} {name or 'plain'}"
            print(f"{what}: visited-set level per query {np.bincount(per_query[:, 3], minlength=3).tolist()}, least evaluations {int(ost[:, 0].min())}")
            assert (per_query[:, 3] == 2).all(), what  # 0 LDS, 1 pool 1, 2 pool 2
            assert (per_query[:, :3] == ost[:, :3]).all(), what
            assert (dk.to_host() == gk).all() and (dd.to_host().view(np.uint32) == gd.view(np.uint32)).all() and (dc.to_host() == gc).all(), what
            assert st["n_table_overflow"] == nq, what
    finally:
        c.s.close()
        _knob(la, monkeypatch, "LEANN_DEBUG_GPOOL_BITS", None)
        _knob(la, monkeypatch, "LEANN_DEBUG_HASH_BITS", None)


# ---- 3. recompute-on graph kernels wider than 256 features ---------------------------------------------------------------------------
# The widest feature width leann_recompute_create accepts at dims = 128 (recompute.hip): it refuses encode_lds_bytes(hp, dp, fused) =
# 128 (hp + 8) 2 + 3 (dp + 192) 16 2 + 6 128 4 > 160 KiB, with hp = h rounded up to 16 and dp = 128 (one column tile):
# 256 (hp + 8) + 30 720 + 3 072 <= 163 840  <=>  hp <= 500, so hp = 496 (162 816 B) and h = 496; hp = 512 needs 166 912 B.  Wider dims
# only lower the limit, so no h > 512 (T = 4) is accepted at any dims.
WIDEST_H = 496


def _recompute_legs(po, s, Gr, W, Q, fh, n):
    """nq = 64 (16 waves) and 704 (4 waves), unfiltered and under a 10 % shared bitmap: GPU == oracle over the same bytes"""
    k, ef = 10, 64
    bm = np.packbits(np.random.default_rng(7).random(n) < 0.10, bitorder="little")
    PQ = po.project_queries(W, Q, fh)
    for nq in (64, NQ):
        ok, od, oc, ost = Gr.search_batch(PQ[:nq], k, ef, 0, 8)
        s.stats(reset=True)
        gk, gd, gc = s.search_batch(Q[:nq], k, ef)
        st = s.stats()
        assert (oc == k).all() and int(ost[:, 1].sum()) > nq
        assert (gc == oc).all() and (gk == ok).all() and (gd.view(np.uint32) == od.view(np.uint32)).all(), nq
        assert st["n_dist_evals"] == int(ost[:, 0].sum()) and st["n_hops_base"] == int(ost[:, 1].sum()), nq
        assert st["n_hops_upper"] == int(ost[:, 2].sum()), nq
        ok, od, oc, ost = Gr.search_filtered_batch(PQ[:nq], k, ef, bm, 0, 8)
        s.stats(reset=True)
        gk, gd, gc = s.search_filtered_batch(Q[:nq], k, ef, bm)
        st = s.stats()
        assert (oc >= 1).all()
        assert (gc == oc).all() and (gk == ok).all() and (gd.view(np.uint32) == od.view(np.uint32)).all(), nq
        assert st["n_dist_evals"] == int(ost[:, 0].sum()) and st["n_hops_base"] == int(ost[:, 1].sum()), nq
        assert st["n_hops_upper"] == int(ost[:, 2].sum()), nq


@pytest.mark.parametrize("h", [100, 300, 448, WIDEST_H])
def test_recompute_on_wide_features(la, po, gpu, h):
    """h = 100: T = 1 with 208-byte rows and the inline norm; 300 (not a multiple of 64), 448 and 496: T = 2"""
    n, d, deg = 4000, 128, 16
    Lc, chk = la.lib(), la._native.check
    F = po.synth_features(SEED, h, 64, 1.0, 0, 0, n)
    W = po.synth_weights(SEED, h, d)
    Q = po.recompute_encode(po.synth_features(SEED, h, 64, 1.0, 1, 0, NQ), W)
    dF, dW = la.DeviceArray.from_host(F), la.DeviceArray.from_host(W)
    r = C.c_void_p()
    chk(Lc.leann_recompute_create(dF.ptr, n, h, dW.ptr, d, 0, 0, C.byref(r)))
    if h == WIDEST_H:  # the next width that changes the encoder's tile is refused
        r2 = C.c_void_p()
        assert Lc.leann_recompute_create(dF.ptr, n, h + 1, dW.ptr, d, 0, 0, C.byref(r2)) != 0
    hb = C.c_void_p()
    chk(Lc.leann_recompute_build_index(r, 0, deg, 64, C.byref(hb)))
    s = la.BackendSearcher(hb, la.BackendType.Hnsw)
    fh, rb = C.c_uint32(0), C.c_uint32(0)
    chk(Lc.leann_backend_feature_rows_export(hb, C.byref(fh), C.byref(rb), None))
    assert fh.value == h and rb.value == (2 * h + 4 + 7) & ~7
    rows = np.zeros((n, rb.value), np.uint8)
    chk(Lc.leann_backend_feature_rows_export(hb, None, None, rows.ctypes.data))
    assert (np.ascontiguousarray(rows[:, : 2 * h]).view(np.uint16) == F).all()
    assert F[:, 256 * ((h - 1) // 256):].any()  # the last chunk of a row holds data
    g = s.graph_export()
    Gr = po.Graph.from_arrays(np.zeros((n, 1), np.float32), deg, 2 * deg, g["max_level"], g["entry"], g["levels"], g["upper_off"],
                              g["adj0"], g["adjU"])
    Gr.set_features(rows, fh.value, rb.value)
    _recompute_legs(po, s, Gr, W, Q, fh.value, n)
    s.close()
    Lc.leann_recompute_close(r)


def _bf16_to_f32(a):
    return (np.ascontiguousarray(a, np.uint16).astype(np.uint32) << 16).view(np.float32)


def test_v2_file_with_640_features(la, po, gpu, tmp_path):
    """beam_search_feat[_filtered]_kernel<4, 4, 16|4>: no encoder of this library makes rows wider than 496 features, but a version-2
    index file may carry up to 1024.  One written by hand — oracle-built graph over the embeddings, bf16 feature rows with the inline
    norm, the weights as f32 — holds 640 features: three chunks in the four-chunk kernel."""
    n, h, d, deg = 2000, 640, 128, 16
    F = po.synth_features(SEED, h, 64, 1.0, 0, 0, n)
    W = po.synth_weights(SEED, h, d)
    Q = po.recompute_encode(po.synth_features(SEED, h, 64, 1.0, 1, 0, NQ), W)
    Wf = _bf16_to_f32(W)
    raw = _bf16_to_f32(F).astype(np.float64) @ Wf.astype(np.float64)
    norms = np.linalg.norm(raw, axis=1).astype(np.float32)  # ||W^T f||; both sides read these bytes
    assert (norms > 0).all() and F[:, 512:].any()
    E = (raw / norms[:, None]).astype(np.float32)
    G = po.Graph.build_hnsw(E, M=deg, efc=64)
    lv, uo, a0, aU = G.export()
    row_bytes = (2 * h + 4 + 7) & ~7
    rows = np.zeros((n, row_bytes), np.uint8)
    rows[:, : 2 * h] = F.view(np.uint8)
    rows[:, 2 * h: 2 * h + 4] = norms.view(np.uint8).reshape(n, 4)
    write_gx2(tmp_path / "documents.index", 0, d, deg, 2 * deg, G.max_level, G.entry, lv, uo, a0, aU, rows, h, Wf)
    s = la.HnswSearcher.load(str(tmp_path / "documents.leann"), d)
    assert s.len() == n
    Gr = po.Graph.from_arrays(np.zeros((n, 1), np.float32), deg, 2 * deg, G.max_level, G.entry, lv, uo, a0, aU)
    Gr.set_features(rows, h, row_bytes)
    _recompute_legs(po, s, Gr, W, Q, h, n)
    s.close()
