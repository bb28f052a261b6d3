"""-m gpu: graph repair after removals (csrc/consolidate.hip) at the widths, row lengths and states that
tests/test_gpu_delete.py never reaches, and searches on tombstoned and repaired f32 graphs held to the oracle.

Everything is exact.  Rows have coordinates that are multiples of 1/8 with |x| <= 2/8 (tests/consolidate_ref.py), so every distance
is exact in f32 in any summation order and the repaired graph must equal the numpy restatement list for list, ties included; the
searches must equal the oracle's walk over the exported graph in ids, distance bits, counts and summed counters.

Repair parity (test_repair_matches_numpy; the cases and what each must reach are stated in tests/delete_cases.py and asserted on
the reference's counters before any device result is looked at):
  hnsw_m64              wide_repair_kernel with alpha = 0; prune_core<NCWIDE>'s second register per lane (my1, s_sel[tid + 64]) and
                        repair_one's write-back `new_adj[lp + j] = c_id[s_sel[j]]` for j in 64..127: level-0 lists of 128 ids; the upper
                        levels run at W = 64 under NC = 256 (`wide` is taken once per handle), lists of 64
  hnsw_m64_mixed        the same write-back for kept counts strictly between 64 and 128 (and below, and of exactly 64)
  vamana_r128[_one_stage]  the widest lists, both prune forms, full lists from the second stage; one node whose 128 ids are all
                        removed: s_nsrc = 129 fills s_src[129], 16 512 slots = 65 chunks of 256
  vamana_r64 / _r65     `wide = max(M0, M) > 64`: the last narrow width (NC = 128) and the first wide one; 65 is no multiple of 4, so
                        lists start off 16 bytes; r65 removes 6 % so that pools stay under NC as well
  hnsw_m8_d1536         `for (j = 4 * tid; j < ld; j += 1024)`: the second trip of the x_p staging; T = 6 slabs in the distance loop;
                        gram_lower<2 / 4 / 8> by pool size (<= 32, <= 64, above)
  vamana_r32_d4096      the longest row the API takes: four staging trips, T = 16, pools cut at NC = 128
  vamana_r96_d1100      ld = 1100: past 1024, `j < ld` false inside the last slab (lanes 19..63 of slab 4), off the 16- and 32-float
                        staging pieces of gram_lower, in the wide kernel; one hand-built node with nc == 0
  hnsw_m8_d30 / _d100   dims no multiple of 4 (ld = 32, zero padded) and ld = 100
  hnsw_m8_60 / _90      60 % / 90 % removed: small pools on every level, pools of one id and of none, chunks with nothing live in
                        them (`if (!__syncthreads_or(any)) continue`)
  hnsw_m8_d100 is made with key_offset = 1 000 000 and removed by global keys.
States (n = 515, d = 40): everything removed; all but three removed; every node of the upper levels removed (`max_level` follows
the new entry down to 0); two rounds of remove + consolidate, each held to the reference applied to the previous result.
Searches (test_searches_match_the_oracle): and_live_kernel with a shared bitmap and with one per query (`b = i % stride`, rows
longer than the bitmap), the live mask's tail bits at n % 8 != 0, the filtered walk while repairs are pending, the plain kernel on
the repaired graph with its replaced entry point, and the exact scan under live AND a per-query bitmap."""
import numpy as np
import pytest

import consolidate_ref as cr
import delete_cases as dc
from test_gpu_delete import U64MAX, _device_search, _exact, _searcher

pytestmark = pytest.mark.gpu

EMPTY = cr.EMPTY


def _grid(rng, n, d):
    return (rng.integers(-2, 3, (n, d)) / 8.0).astype(np.float32)


def _round(s, g, newly, removed, want, key_offset=0):
    """remove `newly` (positions) from searcher s, whose graph is g, consolidate, and hold the result to `want` (the reference's
    graph for `removed`, which includes `newly`): the assertions of test_gpu_delete.py::test_consolidate_matches_numpy_bit_for_bit"""
    n = len(removed)
    keys = np.flatnonzero(newly).astype(np.uint64) + np.uint64(key_offset)
    assert s.remove(keys) == len(keys) and s.live_len() == n - int(removed.sum()) and s.len() == n
    bm, pend = s.removed_bitmap()
    assert (np.unpackbits(bm, bitorder="little")[:n].astype(bool) == removed).all() and not (bm[-1] >> (n & 7) if n & 7 else 0)
    assert pend == cr.pending(g, removed)
    s.consolidate()
    got = s.graph_export()
    assert got["entry"] == want["entry"] and got["max_level"] == want["max_level"]
    bad0 = np.flatnonzero((got["adj0"] != want["adj0"]).any(axis=1))
    assert bad0.size == 0, f"{bad0.size} level-0 lists differ, first nodes {bad0[:5]}: {got['adj0'][bad0[0]]} != {want['adj0'][bad0[0]]}"
    badU = np.flatnonzero((got["adjU"] != want["adjU"]).any(axis=1)) if want["adjU"].size else np.zeros(0, int)
    assert got["adjU"].shape == want["adjU"].shape and badU.size == 0, f"{badU.size} upper lists differ, first rows {badU[:5]}"
    assert (got["adj0"][removed] == EMPTY).all()
    l0 = g["adj0"]
    clean = ~removed & ~(removed[np.where(l0 == EMPTY, 0, l0)] & (l0 != EMPTY)).any(axis=1)
    assert (got["adj0"][clean] == l0[clean]).all()
    live_lists = got["adj0"][~removed]
    assert not removed[live_lists[live_lists != EMPTY]].any()
    assert s.removed_bitmap()[1] == 0
    s.consolidate()                                             # a second pass finds nothing to do
    again = s.graph_export()
    assert (again["adj0"] == want["adj0"]).all() and (again["adjU"] == want["adjU"]).all()
    assert again["entry"] == want["entry"] and again["max_level"] == want["max_level"]
    return clean


@pytest.mark.parametrize("name", list(dc.CASES))
def test_repair_matches_numpy(la, gpu, monkeypatch, name):
    c = dc.CASES[name]
    g, removed, special = dc.graph(name)
    want = dc.reference(name)
    dc.check_needs(name, want)                                  # the case reaches what it is there for, or nothing below counts
    monkeypatch.setenv("LEANN_VAMANA_TWO_STAGE", "1" if c["two_stage"] else "0")
    s = _searcher(la, g, key_offset=c["key_offset"])
    if c["key_offset"]:
        with pytest.raises(la.LeannError):
            s.remove(np.array([3], np.uint64))                  # a position is not a key of this handle
        assert s.live_len() == c["n"]
    clean = _round(s, g, removed, removed, want, key_offset=c["key_offset"])
    assert clean.sum() >= 8
    got = s.graph_export()
    if "empty_pool" in special:
        assert (got["adj0"][special["empty_pool"]] == EMPTY).all()
    if "full_dead" in special:
        l = got["adj0"][special["full_dead"]]
        assert l[0] != EMPTY and not removed[l[l != EMPTY]].any()
    s.close()


# ---- states ---------------------------------------------------------------------------------------------------------------------

N_STATE, D_STATE = 515, 40


def _state_graph(seed, kind="hnsw"):
    rng = np.random.default_rng(seed)
    if kind == "hnsw":
        return cr.random_graph(rng, "hnsw", N_STATE, D_STATE, 8, 16, 2), rng
    return cr.random_graph(rng, "diskann", N_STATE, D_STATE, 24, 24, 0), rng


def test_everything_removed(la, gpu):
    g, rng = _state_graph(21)
    n, k, ef = N_STATE, 10, 48
    Q = _grid(rng, 24, D_STATE)
    removed = np.ones(n, bool)
    s = _searcher(la, g)
    assert s.remove(np.arange(n, dtype=np.uint64)) == n and s.live_len() == 0 and s.len() == n
    ones = np.full((n + 7) // 8, 0xFF, np.uint8)
    per_query = np.full((len(Q), 80), 0xFF, np.uint8)

    def nothing_comes_back():
        k1, d1 = s.search(Q[0], k, ef)
        assert len(k1) == 0 and len(d1) == 0
        k1, _ = s.search_filtered(Q[1], k, ef, ones)
        assert len(k1) == 0
        flt = s.register_filter(ones)
        assert flt.count() == 0
        results = [s.search_batch(Q, k, ef), _device_search(la, s, Q, k, ef), s.search_filtered_batch(Q, k, ef, ones),
                   s.search_filtered_batch(Q, k, ef, per_query), _device_search(la, s, Q, k, ef, allow=ones),
                   s.search_filtered_exact_batch(Q, k, ones), s.search_filtered_exact_batch(Q, k, per_query),
                   _device_search(la, s, Q, k, ef, allow=ones, exact=True)]
        results += [s.search_filter_batch(Q, k, ef, flt, mode) for mode in ("walk", "exact", "auto")]
        flt.close()
        for i, (keys, _, counts) in enumerate(results):
            assert (counts == 0).all() and (keys == U64MAX).all(), f"entry point {i}"

    nothing_comes_back()                                        # tombstones only
    want = cr.consolidate(g, removed)
    assert want["entry"] == g["entry"] and want["max_level"] == g["max_level"]
    _round(s, g, np.zeros(n, bool), removed, want)
    got = s.graph_export()
    assert (got["adj0"] == EMPTY).all() and (got["adjU"] == EMPTY).all()
    assert got["entry"] == g["entry"] and got["max_level"] == g["max_level"]
    nothing_comes_back()                                        # and after the repair, which left nothing
    s.close()


def test_all_but_three_removed(la, gpu):
    g, rng = _state_graph(22)
    removed = np.ones(N_STATE, bool)
    keep = rng.choice(np.flatnonzero(g["levels"] == 0), 3, replace=False)
    removed[keep] = False
    g["adj0"][keep[0], :2] = keep[1:]                           # the three name each other (and removed ids): lists of 1 or 2 survive
    g["adj0"][keep[1], 0] = keep[2]
    want = cr.consolidate(g, removed)
    assert want["max_level"] == 0 and want["entry"] == keep.min() and want["counters"]["repairs"] == 3
    s = _searcher(la, g)
    _round(s, g, removed, removed, want)
    kb, db, cb = s.search_batch(_grid(rng, 24, D_STATE), 10, 48)
    assert (cb <= 3).all() and np.isin(kb[kb != U64MAX], keep).all()
    s.close()


def test_upper_levels_removed(la, po, gpu):
    g, rng = _state_graph(23)
    removed = g["levels"] >= 1
    assert removed[g["entry"]] and 0 < removed.sum() < N_STATE
    want = cr.consolidate(g, removed)
    assert want["max_level"] == 0 and want["entry"] == np.flatnonzero(~removed)[0] and (want["adjU"] == EMPTY).all()
    s = _searcher(la, g)
    _round(s, g, removed, removed, want)
    got = s.graph_export()
    assert got["max_level"] == 0 and (got["adjU"] == EMPTY).all()
    # the plain kernel starts at the new entry on level 0: the oracle's walk over the exported graph, which is told max_level = 0
    Q = _grid(rng, 24, D_STATE)
    G = po.Graph.from_arrays(g["X"], g["M"], g["M0"], got["max_level"], got["entry"], got["levels"], got["upper_off"], got["adj0"], got["adjU"])
    ok, od, oc, _ = G.search_batch(Q, 10, 48, 0, nthreads=8)
    gk, gd, gc = s.search_batch(Q, 10, 48)
    assert (gc == oc).all() and (gk == ok).all() and (gd.view(np.uint32) == od.view(np.uint32)).all()
    s.close()


@pytest.mark.parametrize("kind", ["hnsw", "diskann"])
def test_two_rounds(la, gpu, kind):
    g, rng = _state_graph(24, kind)
    n = N_STATE
    first = rng.random(n) < 0.25
    first[g["entry"]] = True
    want1 = cr.consolidate(g, first)
    assert want1["entry"] != g["entry"]
    second = ~first & (rng.random(n) < 0.15)
    second[want1["entry"]] = True                               # the entry point is replaced in both rounds
    both = first | second
    want2 = cr.consolidate(want1, both)
    assert want2["entry"] not in (g["entry"], want1["entry"]) and want2["counters"]["repairs"] > 0
    s = _searcher(la, g)
    _round(s, g, first, first, want1)
    _round(s, want1, second, both, want2)
    s.close()


# ---- searches on tombstoned and repaired f32 graphs against the oracle -------------------------------------------------------

N_SEARCH, STRIDE = 1499, 208                                    # ceil(1499 / 8) = 188 < 208 = 13 * 16


def _oracle(po, g, ex):
    return po.Graph.from_arrays(g["X"], g["M"], g["M0"], ex["max_level"], ex["entry"], ex["levels"], ex["upper_off"], ex["adj0"], ex["adjU"])


def _eq(got, want, what):
    assert (got[2] == want[2]).all(), f"{what}: counts differ in {(got[2] != want[2]).sum()} queries"
    assert (got[0] == want[0]).all(), f"{what}: ids differ in {(got[0] != want[0]).any(axis=1).sum()} of {len(got[0])} queries"
    assert (got[1].view(np.uint32) == want[1].view(np.uint32)).all(), f"{what}: distance bits differ"


def _walk(s, call, want, what):
    """a device walk and the oracle's: ids, f32 distance bits, counts, and the summed n_dist_evals / n_hops_base"""
    s.stats(reset=True)
    got = call()
    st = s.stats()
    _eq(got, want, what)
    assert st["n_dist_evals"] == int(want[3][:, 0].sum()) and st["n_hops_base"] == int(want[3][:, 1].sum()), what


def _exact_per_query(X, Q, k, ok_rows):
    out = [_exact(X, Q[i: i + 1], k, ok_rows[i]) for i in range(len(Q))]
    return tuple(np.concatenate([o[j] for o in out]) for j in range(3))


def _check_state(po, s, g, removed, Q, allowed, allowed_q, per_query, state):
    """every comparison of one state; the oracle walks the bytes the device holds (graph_export)"""
    n, algo = len(removed), 0 if g["kind"] == "hnsw" else 1
    pend = s.removed_bitmap()[1]
    G = _oracle(po, g, s.graph_export())
    live = ~removed
    live_bm = np.packbits(live, bitorder="little")
    for k, ef in ((10, 48), (1, 1)):
        what = f"{g['kind']} {state} nq={len(Q)} k={k} ef={ef}"
        if pend:    # the filtered kernel under the live mask
            _walk(s, lambda: s.search_batch(Q, k, ef), G.search_filtered_batch(Q, k, ef, live_bm, algo, nthreads=8), what + " unfiltered")
        else:       # the plain kernel
            _walk(s, lambda: s.search_batch(Q, k, ef), G.search_batch(Q, k, ef, algo, nthreads=8), what + " unfiltered, plain")
        shared = np.packbits(allowed, bitorder="little")
        _walk(s, lambda: s.search_filtered_batch(Q, k, ef, shared),
              G.search_filtered_batch(Q, k, ef, np.packbits(allowed & live, bitorder="little"), algo, nthreads=8), what + " shared bitmap")
        _walk(s, lambda: s.search_filtered_batch(Q, k, ef, per_query),
              G.search_filtered_batch(Q, k, ef, np.packbits(allowed_q & live, axis=1, bitorder="little"), algo, nthreads=8),
              what + " one bitmap per query")
        _eq(s.search_filtered_exact_batch(Q, k, per_query), _exact_per_query(g["X"], Q, k, allowed_q & live), what + " exact, per query")


@pytest.mark.parametrize("nq", [24, 600])
@pytest.mark.parametrize("kind", ["hnsw", "diskann"])
def test_searches_match_the_oracle(la, po, gpu, kind, nq):
    n = N_SEARCH
    rng = np.random.default_rng(31)
    g = cr.random_graph(rng, kind, n, 40, 8, 16, 2) if kind == "hnsw" else cr.random_graph(rng, kind, n, 40, 24, 24, 0)
    Q = _grid(rng, nq, 40)
    removed = rng.random(n) < 0.25
    removed[g["entry"]] = True
    allowed = rng.random(n) < 0.5
    allowed[np.flatnonzero(removed)[:60]] = True                # the caller's bitmaps allow removed positions too
    allowed_q = rng.random((nq, n)) < 0.5
    allowed_q[:, np.flatnonzero(removed)[:60]] = True
    # rows of STRIDE bytes: the bits past n in the last byte of the bitmap are set, the bytes past it are non-zero
    per_query = rng.integers(1, 256, (nq, STRIDE)).astype(np.uint8)
    per_query[:, : (n + 7) // 8] = np.packbits(allowed_q, axis=1, bitorder="little")
    per_query[:, (n + 7) // 8 - 1] |= 0xFF << (n & 7) & 0xFF
    s = _searcher(la, g)
    args = (Q, allowed, allowed_q, per_query)
    assert s.remove(np.flatnonzero(removed).astype(np.uint64)) == removed.sum() and s.removed_bitmap()[1] > 0
    _check_state(po, s, g, removed, *args, "repairs pending, entry removed")
    s.consolidate()
    assert s.removed_bitmap()[1] == 0 and s.graph_export()["entry"] != g["entry"]
    _check_state(po, s, g, removed, *args, "consolidated")
    more = rng.choice(np.flatnonzero(~removed), 150, replace=False)
    removed[more] = True
    assert s.remove(more.astype(np.uint64)) == 150 and s.removed_bitmap()[1] > 0
    _check_state(po, s, g, removed, *args, "second removal pending on the repaired graph")
    s.close()
