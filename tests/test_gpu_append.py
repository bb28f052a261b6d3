"""-m gpu: leann_backend_append / leann_backend_append_device — a NEW handle that continues the build of an open one
(include/leann_backend.h "appending to a handle", csrc/build.hip: continue_build, DESIGN.md §5 "Append to a handle").

The builder takes no atomics that decide content, so on rows whose dot products are exact in f32 (build_ref.grid_rows) the result is
held list for list to three references: the file twin (leann_backend_add, the path that existed before), build_ref's restatement
of it, and tests/append_ref.py, the restatement of the definition for what the file twin cannot do (Vamana, levels that are not the
builder's hash).  Searches on the result are held to the oracle walking the exported graph, bit for bit.  Inexact, realistic rows keep
a quality bar: recall@10 of build-2000-append-1000 >= recall@10 of the one-shot build of the 3 000 rows - 0.01, the margin
test_gpu_builder_quality.py gives the builder for running another batch schedule than its reference."""
import ctypes as C

import numpy as np
import pytest

import append_ref as ar
import build_ref as br
import consolidate_ref as cr
from util import SEED, recall_at_k, synth

pytestmark = pytest.mark.gpu

EMPTY = br.EMPTY
NO_KEY = np.iinfo(np.uint64).max
INVALID, UNSUPPORTED = 1, 5
K = 10


# ---- helpers -------------------------------------------------------------------------------------------------------------------------
def _upload(la, X, ld=None, fill=0.0):
    """rows on the device at pitch ld (default: d rounded up to 4 floats); the padding holds `fill`"""
    n, d = X.shape
    ld = ld or (d + 3) & ~3
    Xp = np.full((n, ld), fill, np.float32)
    Xp[:, :d] = X
    return la.DeviceArray.from_host(Xp), ld


def _bt(la, kind):
    return la.BackendType.Hnsw if kind == br.HN else la.BackendType.DiskAnn


def _build(la, kind, X, M, efc, **kw):
    dX, ld = _upload(la, X)
    s = la.BackendSearcher.build_device(_bt(la, kind), dX.ptr, X.shape[0], X.shape[1], ld, M, efc, take_copy=True, **kw)
    return s


def _append_device(la, s, Xnew, ld=None, fill=0.0):
    dN, ld = _upload(la, Xnew, ld, fill)
    return s.append_device(dN.ptr, Xnew.shape[0], ld)


def _diff(ref, g):
    """-> list of complaints (test_gpu_build_parity's comparison, restated)"""
    out = []
    for k in ("entry", "max_level"):
        if int(ref[k]) != int(g[k]):
            out.append(f"{k}: device {g[k]} != reference {ref[k]}")
    for k in ("levels", "upper_off"):
        if not np.array_equal(ref[k], g[k]):
            out.append(f"{k} differ")
    if out:
        return out
    n = len(ref["levels"])
    bad0 = np.flatnonzero((ref["adj0"] != g["adj0"]).any(1))
    if bad0.size:
        out.append(f"level 0: {bad0.size} of {n} lists differ, first {bad0[:4].tolist()}; node {bad0[0]}: device "
                   f"{g['adj0'][bad0[0]][g['adj0'][bad0[0]] != EMPTY].tolist()} reference "
                   f"{ref['adj0'][bad0[0]][ref['adj0'][bad0[0]] != EMPTY].tolist()}")
    if ref["adjU"].shape != g["adjU"].shape:
        out.append(f"adjU shapes differ: {g['adjU'].shape} != {ref['adjU'].shape}")
    elif (ref["adjU"] != g["adjU"]).any():
        out.append(f"upper lists: {int((ref['adjU'] != g['adjU']).any(1).sum())} of {len(ref['adjU'])} differ")
    return out


def _same_export(a, b):
    for k in ("n", "dims", "M", "M0", "max_level", "entry", "n_upper_lists"):
        assert a[k] == b[k], k
    for k in ("levels", "upper_off", "adj0", "adjU"):
        assert a[k].shape == b[k].shape and (a[k] == b[k]).all(), k


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
    return dk.to_host(), dd.to_host(), dc.to_host(), (None if exact else ds.to_host())


def _same_answers(a, b):
    return all((x == y).all() for x, y in zip(a, b))


def _grid_queries(seed, nq, d):
    return (np.random.default_rng(seed).integers(-2, 3, (nq, d)) / 8.0).astype(np.float32)


# ---- 1. HNSW, builder-made: the file twin, the restatement, the rows, the source ------------------------------------------------------
class _Hnsw:
    """hnsw_m8's rows: 800 built on the device, 400 appended through append_device"""

    def __init__(self, la):
        c = br.CASES["hnsw_m8"]
        self.c, self.X, self.n_old = c, br.case_rows(c), 800
        self.Q = _grid_queries(77, 641, c["d"])
        self.src = _build(la, br.HN, self.X[: self.n_old], c["M"], c["efc"])
        self.g_old = self.src.graph_export(with_vectors=True)
        self.src_answers = self.src.search_batch(self.Q[:64], K, 48)
        # the new rows arrive at another pitch than the handle's, with junk in their padding: only `dims` floats per row are taken
        self.new = _append_device(la, self.src, self.X[self.n_old:], ld=48, fill=np.nan)
        self.g = self.new.graph_export(with_vectors=True)


@pytest.fixture(scope="module")
def hnsw(la, gpu):
    h = _Hnsw(la)
    yield h
    h.new.close()
    h.src.close()


def test_hnsw_append_equals_the_file_twin_and_the_restatement(la, po, hnsw, tmp_path):
    h, c = hnsw, hnsw.c
    n_old, n, d = h.n_old, c["n"], c["d"]
    assert h.new.len() == h.new.live_len() == n and h.src.len() == n_old and type(h.new) is type(h.src)
    # the file twin on the same rows: build 800 -> add_to_index 400 -> load -> export
    stem = str(tmp_path / "documents.leann")
    b = la.BackendBuilder(la.BackendType.Hnsw)
    b.build(h.X[:n_old], [], stem, d, c["M"], c["efc"])
    b.add_to_index(h.X[n_old:], stem, d, n_old)
    f = la.HnswSearcher.load(stem, d)
    twin = f.graph_export()
    f.close()
    _same_export(h.g, twin)
    # the restatement, continued from the source's own export
    ref = br.BuildRef(po, br.HN, h.X, c["M"], c["efc"]).continue_from(h.g_old, n_old)
    cn = ref["counters"]
    print("append", {k: v for k, v in cn.items() if v}, "batches", ref["batches"])
    assert cn["prunes_merge"] > 0 and cn["prunes_upper"] > 0 and cn["appends_list"] > 0
    assert ref["batches"][0] == n_old // 8
    dd = _diff(ref, h.g)
    assert not dd, "\n".join(dd)
    assert (h.g["adj0"][:n_old] != h.g_old["adj0"]).any()       # the appended rows did rewrite lists of the first build
    # rows: the source's, then the new ones
    assert (h.g["vectors"].view(np.uint32) == h.X.view(np.uint32)).all()
    # the host-pointer entry point makes the same handle
    t = h.src.append(h.X[n_old:])
    _same_export(t.graph_export(), h.g)
    t.close()
    # the source is as it was
    again = h.src.graph_export(with_vectors=True)
    _same_export(again, h.g_old)
    assert (again["vectors"].view(np.uint32) == h.g_old["vectors"].view(np.uint32)).all()
    assert _same_answers(h.src.search_batch(h.Q[:64], K, 48), h.src_answers)


# ---- 2. searches on the result equal the oracle bit for bit ----------------------------------------------------------------------------
def test_searches_on_the_result_equal_the_oracle(la, po, hnsw):
    h, g, c = hnsw, hnsw.g, hnsw.c
    G = po.Graph.from_arrays(h.X, c["M"], 2 * c["M"], g["max_level"], g["entry"], g["levels"], g["upper_off"], g["adj0"], g["adjU"])
    for nq in (64, 641):                                        # both loop forms
        for ef in (10, 48):
            ok, od, oc, ost = G.search_batch(h.Q[:nq], K, ef, 0, nthreads=8)
            gk, gd, gc, gs = _dev(la, h.new, h.Q[:nq], K, ef)
            assert (gc == oc).all() and (gk == ok).all() and (gd.view(np.uint32) == od.view(np.uint32)).all()
            assert (gs[:, :3] == ost).all() and (gs[:, 3] == 0).all()
            assert (gk[gk != NO_KEY] >= h.n_old).any()          # appended rows are among the answers
    ok, od, oc, _ = G.search_batch(h.Q[:1], K, 48, 0)
    k1, d1 = h.new.search(h.Q[0], K, 48)                        # the single-query call
    assert len(k1) == oc[0] and (k1 == ok[0, : oc[0]]).all() and (d1.view(np.uint32) == od[0, : oc[0]].view(np.uint32)).all()
    hk, hd, hc = h.new.search_batch(h.Q[:64], K, 48)            # the host-pointer batch
    ok, od, oc, _ = G.search_batch(h.Q[:64], K, 48, 0, nthreads=8)
    assert (hk == ok).all() and (hd.view(np.uint32) == od.view(np.uint32)).all() and (hc == oc).all()


# ---- 3. Vamana -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_old,one_stage", [("vamana_r24", 1000, False), ("vamana_r24", 1000, True), ("vamana_r96_wide", 1000, False)])
def test_vamana_append_equals_the_restatement(la, po, gpu, monkeypatch, name, n_old, one_stage):
    c = br.CASES[name]
    X = br.case_rows(c)
    if one_stage:
        monkeypatch.setenv("LEANN_VAMANA_TWO_STAGE", "0")      # read when the SOURCE is built, recorded in the handle ...
    src = _build(la, br.VA, X[:n_old], c["M"], c["efc"])
    if one_stage:
        monkeypatch.delenv("LEANN_VAMANA_TWO_STAGE")           # ... and not read again by the append
        la.lib().leann_debug_reload_env()
    g_old = src.graph_export()
    new = _append_device(la, src, X[n_old:])
    g = new.graph_export()
    ref = ar.AppendRef(po, br.VA, X, c["M"], c["efc"], g_old, two_stage=not one_stage).run()
    cn = ref["counters"]
    print(name, "one-stage" if one_stage else "two-stage", {k: v for k, v in cn.items() if v}, "batches", ref["batches"])
    assert cn["appends_pend"] > 0 and cn["prunes_merge"] > 0 and cn["flushed"] > 0  # the pending area and the final flush ran
    if c["M"] > 64:
        assert cn["kept_gt64"] > 0                             # the wide merge kernel's own ground
    assert ref["batches"][0] == n_old // 8
    assert g["entry"] == g_old["entry"] and g["max_level"] == 0  # the medoid stays
    dd = _diff(ref, g)
    assert not dd, "\n".join(dd)
    assert (g["adj0"][:n_old] != g_old["adj0"]).any()
    if one_stage:                                              # the other form would have made another graph ...
        other = ar.AppendRef(po, br.VA, X, c["M"], c["efc"], g_old, two_stage=True).run()
        assert (other["adj0"] != ref["adj0"]).any(1).sum() > 100
        monkeypatch.setenv("LEANN_VAMANA_TWO_STAGE", "1")      # ... and asking for it in the environment changes nothing
        t = _append_device(la, src, X[n_old:])
        _same_export(t.graph_export(), g)
        t.close()
    _same_export(src.graph_export(), g_old)
    new.close()
    src.close()


# ---- 4. foreign levels: remove -> consolidate -> compact -> append -----------------------------------------------------------------------
def test_append_to_a_compacted_handle_continues_its_lists(la, po, gpu):
    c = br.CASES["hnsw_m8"]
    X = br.case_rows(c)
    n, d, n_add = c["n"], c["d"], 300
    rng = np.random.default_rng(4)
    s = _build(la, br.HN, X, c["M"], c["efc"])
    removed = rng.random(n) < 0.15
    s.remove(np.flatnonzero(removed).astype(np.uint64))
    s.consolidate()
    t, m = s.compact()
    live = t.len()
    assert live == n - removed.sum()
    gc = t.graph_export(with_vectors=True)
    hashed = np.array([po.lib().orc_level(br.LEVEL_SEED, i, c["M"]) for i in range(live)], np.uint8)
    assert (gc["levels"] != hashed).any()                      # the compacted levels are not the builder's hash: the file twin rebuilds here
    Xn = br.grid_rows(4242, n_add, d)
    u = _append_device(la, t, Xn)
    g = u.graph_export(with_vectors=True)
    assert u.len() == u.live_len() == live + n_add
    assert (g["levels"][:live] == gc["levels"]).all()
    assert (g["levels"][live:] == np.array([po.lib().orc_level(br.LEVEL_SEED, i, c["M"]) for i in range(live, live + n_add)], np.uint8)).all()
    assert (g["upper_off"].astype(np.int64) == np.concatenate([[0], np.cumsum(g["levels"].astype(np.int64))[:-1]])).all()
    Xall = np.concatenate([gc["vectors"], Xn])
    assert (g["vectors"].view(np.uint32) == Xall.view(np.uint32)).all()
    ref = ar.AppendRef(po, br.HN, Xall, c["M"], c["efc"], gc).run()
    cn = ref["counters"]
    print("lifecycle", {k: v for k, v in cn.items() if v}, "batches", ref["batches"])
    assert cn["prunes_merge"] > 0 and cn["appends_list"] > 0 and ref["batches"][0] == live // 8
    dd = _diff(ref, g)
    assert not dd, "\n".join(dd)
    # old lists were continued, not rebuilt: an old list is the compacted handle's, or holds a new row, or is what a prune kept of
    # the compacted list and the new rows proposed to it
    old0, new0 = gc["adj0"], g["adj0"][:live]
    same = (old0 == new0).all(1)
    for p in np.flatnonzero(~same):
        a, b = old0[p][old0[p] != EMPTY], new0[p][new0[p] != EMPTY]
        assert np.isin(b[b < live], a).all(), p               # only new rows join an old list; what a prune drops is all that leaves
    nu_old = len(gc["adjU"])
    sameU = (gc["adjU"] == g["adjU"][:nu_old]).all(1)
    print(f"lifecycle: {int(same.sum())} of {live} level-0 lists and {int(sameU.sum())} of {nu_old} upper lists are the compacted handle's")
    assert same.any() and (~same).any()
    _same_export(t.graph_export(), gc)
    # the result can lose rows again
    again = rng.random(live + n_add) < 0.1
    assert u.remove(np.flatnonzero(again).astype(np.uint64)) == again.sum()
    u.consolidate()
    assert u.removed_bitmap()[1] == 0
    v, m2 = u.compact()
    assert v.len() == live + n_add - again.sum()
    for h in (v, u, t, s):
        h.close()


# ---- 5. removals carried ---------------------------------------------------------------------------------------------------------------
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


def _no_removed(keys, counts, removed):
    for i in range(len(keys)):
        assert not removed[keys[i, : counts[i]].astype(np.int64)].any()
        assert (keys[i, counts[i]:] == NO_KEY).all()


def _every_path(la, s, X, Q, removed, rng):
    """every search entry point of the handle: none returns a removed position (test_gpu_delete's sweep, restated)"""
    n, ef = len(X), 48
    allowed = rng.random(n) < 0.5
    allowed[np.flatnonzero(removed)[:50]] = True               # the caller's bitmap allows removed positions
    bm = np.packbits(allowed, bitorder="little")
    ek, ed, ec = _exact(X, Q, K, allowed & ~removed)
    k1, _ = s.search(Q[0], K, ef)
    assert len(k1) and not removed[k1.astype(np.int64)].any()
    kb, db, cb = s.search_batch(Q, K, ef)
    _no_removed(kb, cb, removed)
    assert (cb > 0).all()
    kd, dd, cd, _ = _dev(la, s, Q, K, ef)
    assert (kd == kb).all() and (dd.view(np.uint32) == db.view(np.uint32)).all() and (cd == cb).all()
    kf, df, cf = s.search_filtered_batch(Q, K, ef, bm)
    _no_removed(kf, cf, removed | ~allowed)
    kfd, _, cfd, _ = _dev(la, s, Q, K, ef, allow=bm)
    assert (kfd == kf).all() and (cfd == cf).all()
    k1, _ = s.search_filtered(Q[1], K, ef, bm)
    assert not (removed | ~allowed)[k1.astype(np.int64)].any()
    for got in (s.search_filtered_exact_batch(Q, K, bm), _dev(la, s, Q, K, ef, allow=bm, exact=True)):
        assert (got[2] == ec).all() and (got[0] == ek).all() and (got[1].view(np.uint32) == ed.view(np.uint32)).all()
    flt = s.register_filter(bm)
    assert flt.count() == int((allowed & ~removed).sum())
    for mode in ("walk", "exact", "auto"):
        kr, dr, cr_ = s.search_filter_batch(Q, K, ef, flt, mode)
        _no_removed(kr, cr_, removed | ~allowed)
        if mode == "walk":
            assert (kr == kf).all() and (cr_ == cf).all()
        if mode == "exact":
            assert (kr == ek).all() and (dr.view(np.uint32) == ed.view(np.uint32)).all() and (cr_ == ec).all()
    flt.close()


def test_removals_are_carried_over(la, gpu):
    c = br.CASES["hnsw_m8"]
    X = br.case_rows(c)
    n_old, n = 900, c["n"]
    rng = np.random.default_rng(5)
    Q = _grid_queries(55, 64, c["d"])
    s = _build(la, br.HN, X[:n_old], c["M"], c["efc"])
    gone = rng.random(n_old) < 0.15
    gone[s.graph_export()["entry"]] = True
    assert s.remove(np.flatnonzero(gone).astype(np.uint64)) == gone.sum()
    bm_old, pend_old = s.removed_bitmap()
    assert pend_old > 0                                        # not consolidated
    t = _append_device(la, s, X[n_old:])
    removed = np.concatenate([gone, np.zeros(n - n_old, bool)])
    bm, pend = t.removed_bitmap()
    assert len(bm) == (n + 7) // 8 and (np.unpackbits(bm, bitorder="little")[:n].astype(bool) == removed).all()
    assert t.len() == n and t.live_len() == s.live_len() + (n - n_old) == n - gone.sum()
    g = t.graph_export()
    gd = dict(kind="hnsw", X=X, M=g["M"], M0=g["M0"], max_level=g["max_level"], entry=g["entry"], levels=g["levels"],
              upper_off=g["upper_off"], adj0=g["adj0"], adjU=g["adjU"])
    assert pend == cr.pending(gd, removed) > 0                 # counted again on the device, over the result's lists
    new_lists = g["adj0"][n_old:]
    print(f"removals carried: n_pending {pend_old} -> {pend}; new rows' lists name {int(removed[new_lists[new_lists != EMPTY]].sum())} removed positions")
    _every_path(la, t, X, Q, removed, rng)
    t.consolidate()
    assert t.removed_bitmap()[1] == 0
    g2 = t.graph_export()["adj0"][~removed]
    assert not removed[g2[g2 != EMPTY]].any()
    _every_path(la, t, X, Q, removed, rng)
    assert (s.removed_bitmap()[0] == bm_old).all() and s.removed_bitmap()[1] == pend_old
    t.close()
    s.close()


# ---- 6. row screen ---------------------------------------------------------------------------------------------------------------------
def _search_counted(s, Q, k, ef):
    c0 = s.row_screen_stats()
    s.stats(reset=True)
    keys, dists, counts = s.search_batch(Q, k, ef)
    c1 = s.row_screen_stats()
    return dict(keys=keys, dists=dists, counts=counts, stats=s.stats(), ruled=c1["ruled_out"] - c0["ruled_out"],
                full=c1["read_in_full"] - c0["read_in_full"])


def test_row_screen_planes_are_cut_for_the_result(la, po, gpu, monkeypatch):
    monkeypatch.setenv("LEANN_ROW_SCREEN", "1")
    la.lib().leann_debug_reload_env()
    d, n_old, n_add, nq, M = 768, 2000, 500, 641, 16
    X = synth(po, n_old + n_add, d, n_clusters=2)
    Q = synth(po, nq, d, stream=1, n_clusters=2)
    s = _build(la, br.HN, X[:n_old], M, 64)
    t = _append_device(la, s, X[n_old:])
    on = _search_counted(t, Q, K, 56)                           # the first search screens: the append cut the planes itself
    assert on["ruled"] > 0 and on["ruled"] + on["full"] == on["stats"]["n_dist_evals"] - nq
    assert (on["keys"] >= n_old).any()
    t.set_row_screen(False)
    off = _search_counted(t, Q, K, 56)
    assert off["ruled"] == 0 and off["full"] == 0
    assert (on["counts"] == off["counts"]).all() and (on["keys"] == off["keys"]).all()
    assert (on["dists"].view(np.uint32) == off["dists"].view(np.uint32)).all()
    for f in ("n_dist_evals", "n_hops_base", "n_hops_upper"):
        assert on["stats"][f] == off["stats"][f], f
    g = t.graph_export()
    G = po.Graph.from_arrays(X, M, 2 * M, g["max_level"], g["entry"], g["levels"], g["upper_off"], g["adj0"], g["adjU"])
    ok, od, oc, ost, oruled = G.search_counted_batch(Q, K, 56, 0, nthreads=8)
    assert (on["counts"] == oc).all() and (on["keys"] == ok).all() and (on["dists"].view(np.uint32) == od.view(np.uint32)).all()
    assert on["stats"]["n_dist_evals"] == int(ost[:, 0].sum()) and on["stats"]["n_hops_base"] == int(ost[:, 1].sum())
    assert on["ruled"] == int(oruled.sum()), f"ruled out: device {on['ruled']}, oracle {int(oruled.sum())}"
    t.close()
    s.close()


# ---- 7. quality ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", [(br.HN, 16), (br.VA, 32)])
def test_append_keeps_the_one_shot_builds_recall(la, po, gpu, kind, M):
    """The bar: the one-shot device build of all 3 000 rows, minus the 0.01 that test_gpu_builder_quality.py gives a change of batch
    schedule.  Measured on an MI355X (recall@10, appended / one-shot): HNSW M = 16: 0.9890 / 0.9865 at ef = 32, 0.9975 / 0.9970 at
    ef = 64; Vamana R = 32: 0.9945 / 0.9945 and 1.0000 / 0.9995; no node without an in-edge."""
    n, n_old, d, nq, efc = 3000, 2000, 128, 200, 64
    X, Q = synth(po, n, d), synth(po, nq, d, stream=1)
    dX, dQ = la.DeviceArray.from_host(X), la.DeviceArray.from_host(Q)
    tk, ts, tc = la.DeviceArray((nq, K), np.uint64), la.DeviceArray((nq, K), np.float32), la.DeviceArray(nq, np.uint32)
    la._native.check(la.lib().leann_scan_topk_device(dX.ptr, n, d, d, dQ.ptr, nq, K, None, 0, tk.ptr, ts.ptr, tc.ptr, None))
    la.sync()
    truth = tk.to_host()
    bt = _bt(la, kind)
    whole = la.BackendSearcher.build_device(bt, dX.ptr, n, d, d, M, efc)
    first = la.BackendSearcher.build_device(bt, dX.ptr, n_old, d, d, M, efc)
    grown = first.append_device(dX.ptr + n_old * d * 4, n - n_old, d)
    assert grown.len() == n
    for ef in (32, 64):
        r_whole = recall_at_k(whole.search_batch(Q, K, ef)[0], truth)
        r_grown = recall_at_k(grown.search_batch(Q, K, ef)[0], truth)
        print(f"{kind} M={M} {n_old}+{n - n_old} x {d}: ef={ef}: recall@10 appended {r_grown:.4f} / one-shot {r_whole:.4f}")
        assert r_grown >= r_whole - 0.01
    adj = grown.graph_export()["adj0"]
    valid = adj != EMPTY
    indeg = np.bincount(adj[valid].astype(np.int64), minlength=n)
    print(f"  in-degree 0: {int((indeg == 0).sum())} of {n}, mean out-degree {valid.sum(1).mean():.2f}")
    assert (indeg == 0).mean() < 1e-4                          # every node is reachable from another one
    for h in (grown, first, whole):
        h.close()


# ---- 8. refusals and errors --------------------------------------------------------------------------------------------------------------
def _refused(la, s, code, needle, rows=None, n=4, ld=None, host=False):
    """the call returns `code` with `needle` in its message and makes no handle"""
    L = la.lib()
    out = C.c_void_p(0x1)
    d = s.dims() if s is not None else 40
    ld = ld if ld is not None else (d + 3) & ~3
    buf = la.DeviceArray((4, max(ld, 4)), np.float32)
    hrows = np.zeros((4, d), np.float32)
    if host:
        rc = L.leann_backend_append(s._h if s is not None else None, None if rows == "null" else hrows.ctypes.data_as(la._native.f32p), n, C.byref(out))
    else:
        rc = L.leann_backend_append_device(s._h if s is not None else None, None if rows == "null" else buf.ptr, n, ld, C.byref(out))
    msg = L.leann_last_error().decode()
    assert rc == code and needle in msg, (rc, msg)
    assert not out.value, "a handle was made"


def test_refusals_leave_the_source_as_it_was_and_nothing_behind(la, po, gpu, monkeypatch):
    L, blocks = la.lib(), la.lib().leann_debug_device_blocks
    c = br.CASES["hnsw_m8"]
    X = br.case_rows(c, 600)
    d = c["d"]
    Q = _grid_queries(8, 64, d)
    start = blocks()
    s = _build(la, br.HN, X, c["M"], c["efc"])
    s.search_batch(Q, K, 48)                                   # (the handle's own search scratch exists from here on)
    answers = s.search_batch(Q, K, 48)
    held = blocks()

    def unchanged():
        assert blocks() == held
        assert _same_answers(s.search_batch(Q, K, 48), answers)

    # arguments
    for host in (False, True):
        _refused(la, None, INVALID, "null", host=host)
        _refused(la, s, INVALID, "null", rows="null", host=host)
    assert L.leann_backend_append_device(s._h, 1, 4, d, None) == INVALID and "null" in L.leann_last_error().decode()
    assert L.leann_backend_append(s._h, X.ctypes.data_as(la._native.f32p), 4, None) == INVALID
    _refused(la, s, INVALID, "multiple of 4", ld=d - 4)        # ld < dims
    _refused(la, s, INVALID, "multiple of 4", ld=d + 2)        # ld % 4 != 0
    _refused(la, s, INVALID, "2^31", n=(1 << 31) - 600)        # n_old + n reaches 2^31: refused before a row is read
    unchanged()
    # a bf16 handle
    b = s.to_rows(la.RowType.BF16)
    _refused(la, b, UNSUPPORTED, "leann_backend_build_rows")
    b.close()
    unchanged()
    # a composite handle
    p, q = _build(la, br.HN, X, c["M"], c["efc"]), _build(la, br.HN, X, c["M"], c["efc"], key_offset=len(X))
    comp = la.ShardedIndex.from_searchers([p, q], take_ownership=True).as_backend()
    _refused(la, comp, UNSUPPORTED, "leann_sharded_from_handles")
    comp.close()
    unchanged()
    # a recompute-on handle
    chk = la._native.check
    F, W = po.synth_features(SEED, 64, 64, 1.0, 0, 0, 600), po.synth_weights(SEED, 64, 64)
    dF, dW = la.DeviceArray.from_host(F), la.DeviceArray.from_host(W)
    r, hb = C.c_void_p(), C.c_void_p()
    chk(L.leann_recompute_create(dF.ptr, 600, 64, dW.ptr, 64, 0, 0, C.byref(r)))
    chk(L.leann_recompute_build_index(r, 0, 8, 64, C.byref(hb)))
    feat = la.BackendSearcher(hb, la.BackendType.Hnsw)
    _refused(la, feat, UNSUPPORTED, "leann_recompute_build_index")
    feat.close()
    L.leann_recompute_close(r)
    del dF, dW
    unchanged()
    # a Vamana handle with entry layers
    monkeypatch.setenv("LEANN_VAMANA_NAV", "1")
    v = _build(la, br.VA, X, 24, 48)
    monkeypatch.delenv("LEANN_VAMANA_NAV")
    _refused(la, v, UNSUPPORTED, "LEANN_VAMANA_NAV")
    v.close()
    unchanged()
    # a from_arrays handle whose upper_off is not the prefix sum of its levels (its upper lists stored in another order)
    g = s.graph_export()
    members = np.flatnonzero(g["levels"] > 0)
    uo, aU = g["upper_off"].copy(), g["adjU"].copy()
    off = 0
    for p_ in members[::-1]:                                   # the same lists, laid out from the last node to the first
        lv = int(g["levels"][p_])
        aU[off: off + lv] = g["adjU"][int(g["upper_off"][p_]): int(g["upper_off"][p_]) + lv]
        uo[p_] = off
        off += lv
    f = la.BackendSearcher.from_arrays(la.BackendType.Hnsw, X, g["M"], g["M0"], g["max_level"], g["entry"], g["levels"], uo, g["adj0"], aU)
    mine = blocks()
    _refused(la, f, INVALID, "upper_off")
    assert blocks() == mine
    f.close()
    unchanged()
    # a filter registered on the source belongs to the source: not to a copy of the same length
    flt = s.register_filter(np.full((len(X) + 7) // 8, 0xFF, np.uint8))
    copy = s.append(np.zeros((0, d), np.float32))
    with pytest.raises(la.LeannError, match="filter belongs to another handle") as e:
        copy.search_filter_batch(Q, K, 48, flt, "walk")
    assert e.value.code == INVALID
    s.search_filter_batch(Q, K, 48, flt, "walk")               # still good where it was made
    copy.close()
    flt.close()
    unchanged()
    # a successful append, closed in either order
    for source_first in (False, True):
        a = _build(la, br.HN, X, c["M"], c["efc"])
        base = blocks()
        t = _append_device(la, a, br.grid_rows(9, 100, d))
        assert blocks() > base
        if source_first:
            a.close()
            assert t.search_batch(Q, K, 48)[2].min() > 0       # the result holds nothing of the source's
            t.close()
        else:
            t.close()
            assert blocks() == base
            a.close()
        unchanged()
    s.close()
    assert blocks() == start


# ---- 9. n == 0 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [br.HN, br.VA])
def test_appending_nothing_gives_a_copy(la, gpu, kind):
    c = br.CASES["hnsw_m8" if kind == br.HN else "vamana_r24"]
    X = br.case_rows(c, 500)
    Q = _grid_queries(9, 64, c["d"])
    s = _build(la, kind, X, c["M"], c["efc"], key_offset=1000)
    gone = np.arange(0, 500, 7, dtype=np.uint64) + np.uint64(1000)
    s.remove(gone)
    g = s.graph_export(with_vectors=True)
    h = C.c_void_p()
    la._native.check(la.lib().leann_backend_append_device(s._h, None, 0, c["d"], C.byref(h)))
    a, b = type(s)(h, s.backend_type), s.append(np.zeros((0, c["d"]), np.float32))
    for t in (a, b):
        e = t.graph_export(with_vectors=True)
        _same_export(e, g)
        assert (e["vectors"].view(np.uint32) == g["vectors"].view(np.uint32)).all()
        assert (t.removed_bitmap()[0] == s.removed_bitmap()[0]).all() and t.removed_bitmap()[1] == s.removed_bitmap()[1]
        assert t.live_len() == s.live_len()
        assert _same_answers(t.search_batch(Q, K, 48), s.search_batch(Q, K, 48))  # the keys carry the source's offset
        t.close()
    s.close()
