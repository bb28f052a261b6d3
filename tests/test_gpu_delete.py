"""-m gpu: removing passages from a graph index — tombstones, on-device graph repair, persistence.

Exact parity: rows have coordinates in {-2..2}/8, so every dot product and 1 - dot is exact in f32 in any summation order; the
graph after leann_backend_consolidate must then equal tests/consolidate_ref.py list for list, ties included."""
import ctypes as C
import os

import numpy as np
import pytest

import consolidate_ref as cr
from util import SEED, recall_at_k

pytestmark = pytest.mark.gpu

EMPTY = cr.EMPTY
U64MAX = np.iinfo(np.uint64).max


def _searcher(la, g, key_offset=0):
    kind = la.BackendType.Hnsw if g["kind"] == "hnsw" else la.BackendType.DiskAnn
    return la.BackendSearcher.from_arrays(kind, g["X"], g["M"], g["M0"], g["max_level"], g["entry"], g["levels"], g["upper_off"],
                                          g["adj0"], g["adjU"], key_offset=key_offset)


def _special_nodes(g, removed):
    """node a: its whole list is removed; node b: its candidate set comes out empty (its only neighbour is removed and names
    nothing live but b itself); eight nodes whose lists name no removed id"""
    live = np.flatnonzero(~removed & (g["levels"] == 0))
    dead = np.flatnonzero(removed)
    a, b = int(live[0]), int(live[1])
    g["adj0"][a] = EMPTY
    g["adj0"][a, :5] = dead[:5]
    r = int(dead[5])
    g["adj0"][b] = EMPTY
    g["adj0"][b, 0] = r
    g["adj0"][r] = EMPTY
    g["adj0"][r, :3] = [b, dead[6], dead[7]]
    # nodes whose lists name no removed id (at 30 % removed a random list of 32+ ids is never clean): they must come back byte-identical
    for c in live[2:10]:
        l = g["adj0"][c]
        keep = l[(l != EMPTY) & ~removed[np.where(l == EMPTY, 0, l)]]
        g["adj0"][c] = EMPTY
        g["adj0"][c, : len(keep)] = keep
    return a, b


CASES = {
    # HNSW M = 32: ~19 removed ids per level-0 list -> over 1000 candidates per node, truncated chunk by chunk to NC = 128
    "hnsw_m32": dict(kind="hnsw", d=40, M=32, M0=64, max_level=2, env=None),
    "hnsw_m4_d768": dict(kind="hnsw", d=768, M=4, M0=8, max_level=2, env=None),    # pools <= 32: the small gram tile
    "vamana_r96": dict(kind="diskann", d=256, M=96, M0=96, max_level=0, env=None),  # wide pool, NC = 256, two-stage
    "vamana_r32_one_stage": dict(kind="diskann", d=128, M=32, M0=32, max_level=0, env="0"),
}


@pytest.mark.parametrize("name", list(CASES))
def test_consolidate_matches_numpy_bit_for_bit(la, gpu, monkeypatch, name):
    c = CASES[name]
    n = 2048
    rng = np.random.default_rng(len(name))
    g = cr.random_graph(rng, c["kind"], n, c["d"], c["M"], c["M0"], c["max_level"])
    removed = rng.random(n) < 0.30
    removed[g["entry"]] = True
    a, b = _special_nodes(g, removed)
    before = {k: g[k].copy() for k in ("adj0", "adjU")}
    if c["env"] is not None:
        monkeypatch.setenv("LEANN_VAMANA_TWO_STAGE", c["env"])
    s = _searcher(la, g)
    keys = np.flatnonzero(removed).astype(np.uint64)
    assert s.remove(keys) == len(keys) and s.live_len() == n - len(keys) and s.len() == n
    bm, pend = s.removed_bitmap()
    assert (np.unpackbits(bm, bitorder="little")[:n].astype(bool) == removed).all()
    assert pend == cr.pending(g, removed) > 0
    s.consolidate()
    want = cr.consolidate(g, removed, alpha=1.2, two_stage=c["env"] != "0")
    got = s.graph_export()
    assert got["entry"] == want["entry"] and got["max_level"] == want["max_level"]
    assert not removed[got["entry"]]
    bad0 = np.flatnonzero((got["adj0"] != want["adj0"]).any(axis=1))
    assert bad0.size == 0, f"{bad0.size} level-0 lists differ, first node {bad0[:5]}"
    assert (got["adjU"] == want["adjU"]).all()
    # a node whose list named no removed id is untouched
    l0 = before["adj0"]
    clean = ~removed & ~(removed[np.where(l0 == EMPTY, 0, l0)] & (l0 != EMPTY)).any(axis=1)
    assert clean.sum() >= 8 and (got["adj0"][clean] == l0[clean]).all()
    assert (got["adj0"][removed] == EMPTY).all()
    assert (got["adj0"][b] == EMPTY).all()                      # empty candidate set -> empty list
    assert got["adj0"][a, 0] != EMPTY and not removed[got["adj0"][a][got["adj0"][a] != EMPTY]].any()
    live_lists = got["adj0"][~removed]
    assert not removed[live_lists[live_lists != EMPTY]].any()
    assert s.removed_bitmap()[1] == 0
    s.consolidate()                                             # a second pass finds nothing to do
    assert (s.graph_export()["adj0"] == want["adj0"]).all()
    s.close()


def _exact(X, Q, k, ok_rows, key_offset=0):
    """exact top-k over the rows flagged in ok_rows: ids by (dist, id), f32 distances (exact for the grid rows)"""
    ids = np.flatnonzero(ok_rows)
    keys = np.full((len(Q), k), U64MAX, np.uint64)
    dists = np.full((len(Q), k), np.inf, np.float32)
    counts = np.zeros(len(Q), np.uint32)
    for i, q in enumerate(Q):
        d = (np.float32(1.0) - (X[ids].astype(np.float64) @ q.astype(np.float64)).astype(np.float32)).astype(np.float32)
        o = np.lexsort((ids, d))[:k]
        keys[i, : len(o)] = ids[o] + key_offset
        dists[i, : len(o)] = d[o]
        counts[i] = len(o)
    return keys, dists, counts


def _no_removed(keys, counts, removed, key_offset=0):
    for i in range(len(keys)):
        ids = keys[i, : counts[i]].astype(np.int64) - key_offset
        assert not removed[ids].any()
        assert (keys[i, counts[i]:] == U64MAX).all()


def _device_search(la, s, Q, k, ef, allow=None, exact=False):
    nq = len(Q)
    dq, dk, dd, dc = la.DeviceArray.from_host(Q), la.DeviceArray((nq, k), np.uint64), la.DeviceArray((nq, k), np.float32), \
        la.DeviceArray(nq, np.uint32)
    da = la.DeviceArray.from_host(allow) if allow is not None else None
    if exact:
        s.search_filtered_exact_batch_device(dq.ptr, nq, k, da.ptr, 0, dk.ptr, dd.ptr, dc.ptr)
    elif allow is not None:
        s.search_filtered_batch_device(dq.ptr, nq, k, ef, da.ptr, 0, dk.ptr, dd.ptr, dc.ptr)
    else:
        s.search_batch_device(dq.ptr, nq, k, ef, dk.ptr, dd.ptr, dc.ptr)
    la.sync()
    return dk.to_host(), dd.to_host(), dc.to_host()


def _every_path(la, s, X, Q, removed, rng, key_offset=0):
    n, k, ef = len(X), 10, 48
    allowed = rng.random(n) < 0.5
    allowed[np.flatnonzero(removed)[:50]] = True                # the caller's bitmap allows removed positions
    bm = np.packbits(allowed, bitorder="little")
    ek, ed, ec = _exact(X, Q, k, allowed & ~removed, key_offset)
    # single, batch, device
    k1, _ = s.search(Q[0], k, ef)
    assert len(k1) and not removed[k1.astype(np.int64) - key_offset].any()
    kb, db, cb = s.search_batch(Q, k, ef)
    _no_removed(kb, cb, removed, key_offset)
    assert (cb > 0).all()
    kd, dd, cd = _device_search(la, s, Q, k, ef)
    assert (kd == kb).all() and (dd.view(np.uint32) == db.view(np.uint32)).all() and (cd == cb).all()
    # filtered walk, host and device
    kf, df, cf = s.search_filtered_batch(Q, k, ef, bm)
    _no_removed(kf, cf, removed | ~allowed, key_offset)
    kfd, dfd, cfd = _device_search(la, s, Q, k, ef, allow=bm)
    assert (kfd == kf).all() and (cfd == cf).all()
    k1, _ = s.search_filtered(Q[1], k, ef, bm)
    assert not (removed | ~allowed)[k1.astype(np.int64) - key_offset].any()
    # filtered exact, host and device: numpy's exact top-k over live AND allowed, ids and f32 bits
    for got in (s.search_filtered_exact_batch(Q, k, bm), _device_search(la, s, Q, k, ef, allow=bm, exact=True)):
        assert (got[2] == ec).all() and (got[0] == ek).all() and (got[1].view(np.uint32) == ed.view(np.uint32)).all()
    # registered filter, modes 0 / 1 / 2
    flt = s.register_filter(bm)
    assert flt.count() == int((allowed & ~removed).sum())
    for mode in ("walk", "exact", "auto"):
        kr, dr, cr_ = s.search_filter_batch(Q, k, ef, flt, mode)
        _no_removed(kr, cr_, removed | ~allowed, key_offset)
        if mode == "walk":
            assert (kr == kf).all() and (cr_ == cf).all()
        if mode == "exact":
            assert (kr == ek).all() and (dr.view(np.uint32) == ed.view(np.uint32)).all() and (cr_ == ec).all()
    return flt


def test_no_removed_key_is_ever_returned(la, gpu):
    n, d = 1536, 40
    rng = np.random.default_rng(11)
    g = cr.random_graph(rng, "hnsw", n, d, 8, 16, 2)
    Q = (rng.integers(-2, 3, (24, d)) / 8.0).astype(np.float32)
    s = _searcher(la, g)
    old = s.register_filter(np.full((n + 7) // 8, 0xFF, np.uint8))
    removed = rng.random(n) < 0.25
    removed[g["entry"]] = True
    with pytest.raises(la.LeannError) as e:
        s.remove(np.array([3, n], np.uint64))                   # an unknown key: named, and nothing is applied
    assert str(n) in str(e.value) and s.live_len() == n
    keys = np.flatnonzero(removed).astype(np.uint64)
    assert s.remove(keys) == len(keys)
    assert s.remove(keys[:7]) == 0                              # already removed: ignored, not counted
    with pytest.raises(la.LeannError) as e:
        s.search_filter_batch(Q, 10, 48, old, "walk")
    assert e.value.code == 1 and "filter predates a removal; register it again" in str(e.value)
    old.close()
    assert s.removed_bitmap()[1] > 0
    _every_path(la, s, g["X"], Q, removed, rng).close()         # before the repair: tombstones + filtered walk
    s.consolidate()
    assert s.removed_bitmap()[1] == 0
    flt = _every_path(la, s, g["X"], Q, removed, rng)           # after it: the plain kernel for unfiltered walks
    more = np.flatnonzero(~removed)[:40]
    removed[more] = True
    assert s.remove(more.astype(np.uint64)) == 40               # a second round of removals on a repaired graph
    with pytest.raises(la.LeannError):
        s.search_filter_batch(Q, 10, 48, flt, "exact")
    flt.close()
    _every_path(la, s, g["X"], Q, removed, rng).close()
    s.close()


def test_composite_handle_routes_removals_to_its_shards(la, gpu):
    n0, n1, d = 1024, 768, 40
    rng = np.random.default_rng(5)
    g0, g1 = cr.random_graph(rng, "hnsw", n0, d, 8, 16, 1), cr.random_graph(rng, "hnsw", n1, d, 8, 16, 1)
    X = np.concatenate([g0["X"], g1["X"]])
    Q = (rng.integers(-2, 3, (16, d)) / 8.0).astype(np.float32)
    s = la.ShardedIndex.from_searchers([_searcher(la, g0), _searcher(la, g1, key_offset=n0)], take_ownership=True).as_backend()
    removed = rng.random(n0 + n1) < 0.2
    with pytest.raises(la.LeannError):
        s.remove(np.array([5, n0 + n1], np.uint64))
    assert s.live_len() == n0 + n1
    keys = np.flatnonzero(removed).astype(np.uint64)
    assert s.remove(keys) == len(keys) and s.live_len() == n0 + n1 - len(keys)
    bm, pend = s.removed_bitmap()
    assert (np.unpackbits(bm, bitorder="little")[: n0 + n1].astype(bool) == removed).all() and pend > 0
    allow = np.full((n0 + n1 + 7) // 8, 0xFF, np.uint8)
    ek, ed, ec = _exact(X, Q, 10, ~removed)
    for phase in range(2):
        kb, db, cb = s.search_batch(Q, 10, 48)
        _no_removed(kb, cb, removed)
        kf, df, cf = s.search_filtered_batch(Q, 10, 48, allow)
        _no_removed(kf, cf, removed)
        kx, dx, cx = s.search_filtered_exact_batch(Q, 10, allow)
        assert (cx == ec).all() and (dx.view(np.uint32) == ed.view(np.uint32)).all()
        _no_removed(kx, cx, removed)                            # (entries of equal distance may come in either order across shards)
        flt = s.register_filter(allow)
        for mode in ("walk", "exact", "auto"):
            kr, dr, cr_ = s.search_filter_batch(Q, 10, 48, flt, mode)
            _no_removed(kr, cr_, removed)
        flt.close()
        if phase == 0:
            s.consolidate()
            assert s.removed_bitmap()[1] == 0
            for gi, (g, lo) in enumerate(((g0, 0), (g1, n0))):
                want = cr.consolidate(g, removed[lo: lo + len(g["X"])])
                got = s.shard(gi).graph_export()
                assert (got["adj0"] == want["adj0"]).all() and (got["adjU"] == want["adjU"]).all() and got["entry"] == want["entry"]
    s.close()


def test_handle_without_removals_is_unchanged(la, gpu):
    """zero removals: the same ids, distances and per-query counters as an untouched handle built from the same arrays"""
    n, d = 1536, 40
    rng = np.random.default_rng(3)
    g = cr.random_graph(rng, "hnsw", n, d, 8, 16, 2)
    Q = (rng.integers(-2, 3, (32, d)) / 8.0).astype(np.float32)
    s, t = _searcher(la, g), _searcher(la, g)
    assert s.remove(np.zeros(0, np.uint64)) == 0 and s.live_len() == n
    s.consolidate()
    assert s.removed_bitmap()[1] == 0 and not s.removed_bitmap()[0].any()
    out = []
    for h in (s, t):
        nq, k = len(Q), 10
        dq, dk, dd, dc, ds = la.DeviceArray.from_host(Q), la.DeviceArray((nq, k), np.uint64), la.DeviceArray((nq, k), np.float32), \
            la.DeviceArray(nq, np.uint32), la.DeviceArray((nq, 4), np.uint32)
        h.search_batch_device(dq.ptr, nq, k, 48, dk.ptr, dd.ptr, dc.ptr, ds.ptr)
        la.sync()
        out.append((dk.to_host(), dd.to_host().view(np.uint32), dc.to_host(), ds.to_host()))
    for a, b in zip(*out):
        assert (a == b).all()
    gs, gt = s.graph_export(), t.graph_export()
    assert (gs["adj0"] == gt["adj0"]).all() and (gs["adjU"] == gt["adjU"]).all()
    s.close()
    t.close()


def test_persistence(la, gpu, tmp_path):
    n, d = 1024, 40
    rng = np.random.default_rng(9)
    g = cr.random_graph(rng, "hnsw", n, d, 8, 16, 2)
    Q = (rng.integers(-2, 3, (16, d)) / 8.0).astype(np.float32)
    stem = str(tmp_path / "documents.leann")
    index, side = str(tmp_path / "documents.index"), str(tmp_path / "documents.tombstones")
    s = _searcher(la, g)
    s.save(stem)
    assert not os.path.exists(side)
    plain = open(index, "rb").read()
    removed = rng.random(n) < 0.2
    s.remove(np.flatnonzero(removed).astype(np.uint64))
    s.save(stem)                                                # remove without consolidate: the index file is unchanged
    assert open(index, "rb").read() == plain and os.path.exists(side)
    want = s.search_batch(Q, 10, 48)
    bm, pend = s.removed_bitmap()
    o = la.BackendSearcher.load(la.BackendType.Hnsw, stem, d)
    obm, opend = o.removed_bitmap()
    assert (obm == bm).all() and opend == pend and o.live_len() == s.live_len() == n - int(removed.sum())
    got = o.search_batch(Q, 10, 48)
    assert (got[0] == want[0]).all() and (got[1].view(np.uint32) == want[1].view(np.uint32)).all() and (got[2] == want[2]).all()
    o.close()
    s.close()
    # a damaged sidecar is refused
    raw = open(side, "rb").read()
    for broken in (raw[:-3], raw[:16] + (int.from_bytes(raw[16:24], "little") + 1).to_bytes(8, "little") + raw[24:]):
        open(side, "wb").write(broken)
        with pytest.raises(la.LeannError) as e:
            la.BackendSearcher.load(la.BackendType.Hnsw, stem, d)
        assert e.value.code == 3
    os.remove(side)
    # the file twin: open -> remove -> consolidate -> save
    keys = np.flatnonzero(removed).astype(np.uint64)
    la.BackendBuilder(la.BackendType.Hnsw).remove_from_index(keys, stem, d)
    o = la.BackendSearcher.load(la.BackendType.Hnsw, stem, d)
    assert o.live_len() == n - len(keys) and o.removed_bitmap()[1] == 0
    want = cr.consolidate(g, removed)
    assert (o.graph_export()["adj0"] == want["adj0"]).all()
    kb, _, cb = o.search_batch(Q, 10, 48)
    _no_removed(kb, cb, removed)
    o.close()
    # append after a removal: the old tombstones stay, the new rows are live
    extra = (rng.integers(-2, 3, (64, d)) / 8.0).astype(np.float32)
    la.BackendBuilder(la.BackendType.Hnsw).add_to_index(extra, stem, d, n)
    o = la.BackendSearcher.load(la.BackendType.Hnsw, stem, d)
    bm2, _ = o.removed_bitmap()
    bits = np.unpackbits(bm2, bitorder="little")[: n + 64].astype(bool)
    assert o.len() == n + 64 and (bits[:n] == removed).all() and not bits[n:].any() and o.live_len() == n + 64 - len(keys)
    kb, _, cb = o.search_batch(extra[:8], 1, 64)
    assert (cb == 1).all() and not bits[kb[:, 0].astype(np.int64)].any()
    o.close()
    # nothing removed: a stale sidecar does not survive a save
    t = _searcher(la, g)
    t.save(stem)
    assert not os.path.exists(side)
    t.close()


def _rows(la, n, d, stream):
    buf = la.DeviceArray((n, d), np.float32)
    la._native.check(la.lib().leann_synth_rows_device(SEED, d, d, 64, 256, 1.0, stream, 0, n, buf.ptr, None))
    la.sync()
    return buf


@pytest.mark.parametrize("kind,degree", [("hnsw", 16), ("diskann", 32)])
def test_search_quality_after_repair(la, po, gpu, kind, degree):
    """recall@10 of the plain search at ef = 64 after removing a random 10 % of 20 000 x 64 clustered rows and consolidating, against
    a graph built from scratch on the live rows only (same parameters, same ef).  The margin is twice the spread of the rebuilt
    graph's recall over three row permutations — the builder's own noise.  Asserts consolidated >= rebuilt - margin.
    The figures are printed; none has been recorded from an MI355X run yet."""
    n, d, nq, ef = 20_000, 64, 1000, 64
    bt = la.BackendType.Hnsw if kind == "hnsw" else la.BackendType.DiskAnn
    rng = np.random.default_rng(17)
    dX = _rows(la, n, d, 0)
    X, Q = dX.to_host(), _rows(la, nq, d, 1).to_host()
    removed = np.zeros(n, bool)
    removed[rng.choice(n, n // 10, replace=False)] = True
    live = np.flatnonzero(~removed)
    truth = live[po.exact_topk(X[live], Q, 10)]
    s = la.BackendSearcher.build_device(bt, dX.ptr, n, d, d, degree, 64)
    s.remove(np.flatnonzero(removed).astype(np.uint64))
    s.consolidate()
    assert s.removed_bitmap()[1] == 0
    keys, _, counts = s.search_batch(Q, 10, ef)
    _no_removed(keys, counts, removed)
    r_cons = recall_at_k(keys, truth)
    s.close()
    rebuilt = []
    for perm_seed in range(3):
        perm = live if perm_seed == 0 else np.random.default_rng(perm_seed).permutation(live)
        dL = la.DeviceArray.from_host(X[perm])
        t = la.BackendSearcher.build_device(bt, dL.ptr, len(perm), d, d, degree, 64)
        k2, _, _ = t.search_batch(Q, 10, ef)
        rebuilt.append(recall_at_k(np.where(k2 == U64MAX, -1, perm[np.minimum(k2, len(perm) - 1).astype(np.int64)]), truth))
        t.close()
    margin = 2 * (max(rebuilt) - min(rebuilt))
    print(f"{kind} degree {degree}: recall@10 consolidated {r_cons:.4f}, rebuilt {rebuilt[0]:.4f} (permutations: "
          f"{', '.join(f'{r:.4f}' for r in rebuilt)}), margin {margin:.4f}")
    assert r_cons >= rebuilt[0] - margin


EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "leann-rs_amd", "host", "leann")
TOPICS = ["rust ownership borrow checker lifetimes", "python asyncio event loop coroutine", "vector database embedding search",
          "graph traversal beam hnsw neighbours", "gpu kernel wavefront lds bandwidth", "bm25 ranking term frequency"]


def test_cli_delete(gpu, tmp_path):
    """`leann delete` on the 600 x 96 index of tests/test_gpu_cli.py's recipe: the removed ids vanish from `leann search`"""
    import json
    import subprocess

    def run(*args):
        return subprocess.run([EXE, *args], capture_output=True, text=True)

    docs = [dict(id=str(i + 1), text=f"passage {i} about {TOPICS[i % len(TOPICS)]} number {i * 7919 % 1000}",
                 metadata=dict(source=f"file{i % 10}.{'rs' if i % 2 else 'py'}", lines=i)) for i in range(600)]
    (tmp_path / "docs.jsonl").write_text("\n".join(json.dumps(x) for x in docs))
    idx = str(tmp_path / "idx")
    r = run("build", "--index-dir", idx, "--passages-jsonl", str(tmp_path / "docs.jsonl"), "--dimensions", "96", "--graph-degree", "16",
            "--complexity", "64")
    assert r.returncode == 0, r.stderr
    q = "graph traversal beam hnsw neighbours"
    searches = (("--hybrid",), ("--hybrid", "--bm25", "host"), ("--filter", "source:*.rs"), ("--filter", "source:*.rs", "--device-filter"),
                ("--auto-hybrid", "false"))

    def hits(extra):
        r = run("search", q, "-i", idx, "--top-k", "10", "--format", "json", *extra)
        assert r.returncode == 0, r.stderr
        return [x["id"] for x in json.loads(r.stdout)]

    before = {e: hits(e) for e in searches}
    victims = sorted({i for e in searches for i in before[e][:4]}, key=int)
    assert len(victims) >= 4
    (tmp_path / "ids.txt").write_text("\n".join(victims[2:]) + "\n")
    r = run("delete", idx, "--ids", ",".join(victims[:2]))
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == f"Index '{idx}': removed 2 passages, 598 live"
    r = run("delete", idx, "--ids-file", str(tmp_path / "ids.txt"))
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == f"Index '{idx}': removed {len(victims) - 2} passages, {600 - len(victims)} live"
    r = run("delete", idx, "--ids", "1,no-such-id")
    assert r.returncode != 0 and "no-such-id" in r.stderr
    for e in searches:
        after = hits(e)
        assert len(after) == 10 and not set(after) & set(victims), e
    assert os.path.exists(os.path.join(idx, "documents.tombstones"))
    assert len(open(os.path.join(idx, "documents.ids.txt")).read().split()) == 600   # the id map is not rewritten
