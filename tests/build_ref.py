"""The batched on-device builder (csrc/build.hip: build_on_device / builder_insert_range / select_one / reverse_merge_one) restated
in plain numpy around the oracle's construction walk, for tests/test_gpu_build_parity.py and tests/test_cpu_build_ref.py.

The builder takes no atomics that decide content, so on rows whose dot products are exact in f32 (coordinates that are small
multiples of 1/8: the Gram tile, the wave dot and numpy agree in any summation order) its graph can be restated list for list:

  setup      levels = orc_level(0x5EED0003, i, M) (HNSW, and Vamana under LEANN_VAMANA_NAV; else 0); rows [lo, n) enter in the hash order of insertion_order, the
             medoid (best row by <mean, x>, lower id on ties) pinned first for single-level Vamana; the first point is the entry and is never linked
             by itself.
  per batch  of min(16384, max(1, s / fraction), n - s) points, s = points already in:
             1. every level job (levels max_level .. 1, the batch members of that level, in batch order) and level 0 are searched
                against the graph as it was before the batch (oracle.c: orc_graph_search_level, beam = efc; Vamana also records the
                first 256 nodes expanded);
             2. per level, top first: select — the beam cut to min(count, efc, NC), the point itself dropped, Vamana: the expanded
                nodes beyond the beam's worst key, sorted, evenly subsampled to at most 48, appended behind the beam cut to NC - taken;
                prune (consolidate_ref.prune's rule) to M; the list is written and its tail cleared; every kept neighbour gets a
                proposal (target, dist, source).  Proposals are stably sorted by (target, dist) — equal keys stay in batch order — and
                every target takes its run (at most NC of it), without the proposals whose source its list or pending area already
                holds (refine passes only: a first pass proposes new points): k <= room in the list + room in the pending area -> appended in run
                order, list first; otherwise list + pending + the closest NC - len - pl proposals, sorted by (dist, id), pruned to
                the list width, and the pending area cleared (level 0 of Vamana only holds one);
             3. entry / max_level move to the first point of the batch whose level exceeds max_level.
  afterwards optional refine passes (every point re-linked in ONE batch against the finished graph, LEANN_VAMANA_PASSES), then
             whatever is still pending is folded into its list by one prune per node (alpha 1.2).

`BuildRef(...).build()` returns the graph as a consolidate_ref dict plus `counters` (which paths ran) and `batches`."""
import numpy as np

import consolidate_ref as cr

EMPTY = 0xFFFFFFFF
EXPCAP = 256   # expanded nodes recorded per construction search
PATHMAX = 48   # path nodes that join a Vamana pool
BMAX = 16384   # largest batch
LEVEL_SEED = 0x5EED0003
FULL = np.uint64(0xFFFFFFFFFFFFFFFF)
LOW = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)

COUNTERS = ("pools_le32", "pools_33_64", "pools_gt64", "pools_cut_nc", "appends_list", "appends_pend", "prunes_merge", "prunes_upper",
            "runs_cut", "ties", "path_taken", "path_over_max", "self_removed", "kept_gt64", "pools_gt176", "flushed", "tail_cleared",
            "dup_skipped")


def f32_orderable(d):
    u = np.ascontiguousarray(d, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def orderable_f32(u):
    u = np.ascontiguousarray(u, np.uint32)
    return np.where(u & np.uint32(0x80000000), u & np.uint32(0x7FFFFFFF), ~u).astype(np.uint32).view(np.float32)


def pack(d, ids):
    return (f32_orderable(d).astype(np.uint64) << S32) | np.asarray(ids, np.uint64)


def mix64(x):
    x = np.asarray(x, np.uint64) + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def insertion_order(lo, n, pin_first=None):
    """order[j] = position inserted j-th: [0, lo) in place, [lo, n) sorted by a hash of the position, `pin_first` ahead of them"""
    pos = np.arange(lo, n, dtype=np.uint64)
    keyed = np.sort((mix64(pos ^ np.uint64(0x4F52444552)) & np.uint64(0xFFFFFFFF00000000)) | pos)
    rest = (keyed & LOW).astype(np.uint32)
    if pin_first is not None:
        rest = np.concatenate([np.array([pin_first], np.uint32), rest[rest != pin_first]])
    return np.concatenate([np.arange(lo, dtype=np.uint32), rest])


def batch_sizes(s0, n, fraction, refine=False):
    out, s = [], s0
    while s < n:
        B = min(BMAX, BMAX if refine else max(1, s // fraction), n - s)
        out.append(B)
        s += B
    return out


def medoid(X):
    """-> (row, gap): column means in f64 cast to f32 (bit-equal to the device's on grid rows), best row by <mean, x> in f64, lower
    id on ties; gap = best score - second best (the device's f32 scan reorders a dot worth < 1e-7 here: gap must be >= 1e-6)"""
    mean = (X.astype(np.float64).sum(0) / X.shape[0]).astype(np.float32)
    s = X.astype(np.float64) @ mean.astype(np.float64)
    best = int(np.argmax(s))  # first of equal maxima
    rest = np.delete(s, best)
    return best, float(s[best] - rest.max()) if rest.size else np.inf


def grid_rows(seed, n, d, shape="uniform"):
    """rows whose coordinates are multiples of 1/8 in [-4/8, 4/8]: every dot product of two rows and 1 - dot is exact in f32 in any
    summation order (and the rows are exact in bf16), with plenty of ties.
      uniform  coordinates uniform in {-2..2}/8
      hubs     the same, every 8th row doubled: long rows that draw back-edges from everywhere, so their lists fill, are pruned
               with most of the pool kept, and take runs of proposals longer than the pool has room for
      blocks   16 clusters, each on 4 coordinates of its own ({-2..4}/8, zero elsewhere): rows of different clusters are orthogonal,
               a plateau of distance exactly 1 ordered by id alone, which a construction search crosses by id before it finds the
               point's own cluster — the walks that leave more than PATHMAX expanded nodes behind the beam"""
    rng = np.random.default_rng(seed)
    if shape == "blocks":
        X = np.zeros((n, d), np.int64)
        k = rng.integers(0, 16, n)
        X[np.arange(n)[:, None], (k * (d // 16))[:, None] + np.arange(4)[None, :]] = rng.integers(-2, 5, (n, 4))
    else:
        X = rng.integers(-2, 3, (n, d))
        if shape == "hubs":
            X[::8] *= 2
    return (X / 8.0).astype(np.float32)


def _knob(knobs, name, dflt, lo, hi):
    v = knobs.get(name)
    if v is None or v == "":
        return dflt
    v = int(v)
    return v if lo <= v <= hi else dflt


class BuildRef:
    def __init__(self, po, kind, X, M, complexity, knobs=None, nthreads=8, numpy_prune=False):
        knobs = knobs or {}
        self.po, self.kind, self.hnsw = po, kind, kind == "hnsw"
        self.X = np.ascontiguousarray(X, np.float32)
        self.n, self.d = self.X.shape
        self.M, self.M0 = M, 2 * M if self.hnsw else M
        self.efc = max(complexity, M)
        self.NC = 256 if max(self.M, self.M0) > 64 else 128
        self.alpha = np.float32(1.2)
        self.fraction = _knob(knobs, "LEANN_BUILD_BATCH_FRACTION", 8, 1, 1 << 20)
        self.two_stage = bool(_knob(knobs, "LEANN_VAMANA_TWO_STAGE", 1, 0, 1)) and not self.hnsw
        self.P = 0 if self.hnsw else _knob(knobs, "LEANN_VAMANA_PENDING", 4, 0, 32)
        self.passes = _knob(knobs, "LEANN_VAMANA_PASSES", 1, 1, 3)
        self.leveled = self.hnsw or bool(_knob(knobs, "LEANN_VAMANA_NAV", 0, 0, 1))  # entry layers above a Vamana base graph
        self.alpha1 = np.float32(_knob(knobs, "LEANN_VAMANA_ALPHA1_PCT", int(self.alpha * np.float32(100.0) + np.float32(0.5)), 100, 400)) / np.float32(100.0)
        self.nthreads, self.numpy_prune = nthreads, numpy_prune
        self.c = dict.fromkeys(COUNTERS, 0)
        self.batches = []
        n, nn = self.n, max(self.n, 1)
        lib = po.lib()
        self.levels = np.array([lib.orc_level(LEVEL_SEED, i, M) if self.leveled else 0 for i in range(n)], np.uint8)
        self.upper_off = np.zeros(nn, np.uint32)
        self.upper_off[1:n] = np.cumsum(self.levels.astype(np.uint64))[:-1]
        self.nu = int(self.levels.astype(np.int64).sum())
        self.adj0 = np.full((nn, self.M0), EMPTY, np.uint32)
        self.adjd0 = np.zeros((nn, self.M0), np.float32)
        self.adjU = np.full((max(self.nu, 1), M), EMPTY, np.uint32)
        self.adjdU = np.zeros((max(self.nu, 1), M), np.float32)
        self.pend = np.full((nn, max(self.P, 1)), EMPTY, np.uint32)
        self.pendd = np.zeros((nn, max(self.P, 1)), np.float32)
        self.entry, self.max_level = 0, 0

    # ---- lists -------------------------------------------------------------------------------------
    def _list(self, node, level):
        if level == 0:
            return self.adj0[node], self.adjd0[node]
        r = int(self.upper_off[node]) + level - 1
        return self.adjU[r], self.adjdU[r]

    def _prune(self, cid, cd, limit, alpha, merge):
        nc, c = len(cid), self.c
        c["pools_le32" if nc <= 32 else "pools_33_64" if nc <= 64 else "pools_gt64"] += 1
        c["pools_gt176"] += nc > 176
        if self.numpy_prune:
            kept = np.asarray(cr.prune(self.X, cid.astype(np.int64), cd, limit, alpha, self.two_stage), np.int64)
        else:
            kept = self.po.prune(self.X, cid, cd, limit, alpha, self.two_stage).astype(np.int64)
        c["kept_gt64"] += len(kept) > 64
        return kept

    # ---- select_one --------------------------------------------------------------------------------
    def _select(self, q, level, keys, cnt, exp, nexp, alpha):
        NC, c = self.NC, self.c
        nc = min(int(cnt), self.efc, NC)
        cut = min(int(cnt), self.efc) > NC
        k = keys[:nc]
        me = np.flatnonzero((k & LOW) == np.uint64(q))
        if me.size:  # a point that is already linked finds itself: dropped, the rest moves up
            k = np.delete(k, me[0])
            nc -= 1
            c["self_removed"] += 1
        if exp is not None and nc > 0:
            wmax = k[nc - 1]
            p = exp[: min(int(nexp), EXPCAP)]
            p = np.sort(p[(p != FULL) & (p > wmax)])
            n_path = len(p)
            take = min(n_path, PATHMAX)
            keep = min(nc, NC - take)
            cut = cut or keep < nc
            if take:
                k = np.concatenate([k[:keep], p[(np.arange(take, dtype=np.uint64) * np.uint64(n_path)) // np.uint64(take)]])
            else:
                k = k[:keep]
            c["path_taken"] += take
            c["path_over_max"] += n_path > PATHMAX
        c["pools_cut_nc"] += cut
        cid = (k & LOW).astype(np.uint32)
        cd = orderable_f32((k >> S32).astype(np.uint32))
        kept = self._prune(cid, cd, self.M, alpha, False)
        ids, ds = self._list(q, level)
        ns = len(kept)
        c["tail_cleared"] += int((ids[ns:] != EMPTY).any())
        ids[:ns], ds[:ns] = cid[kept], cd[kept]
        ids[ns:] = EMPTY
        return cid[kept], cd[kept]

    # ---- reverse_merge_one -------------------------------------------------------------------------
    def _merge(self, t, level, srcs, od, alpha, flush=False):
        NC, c = self.NC, self.c
        ids, ds = self._list(t, level)
        cap = len(ids)
        P = self.P if level == 0 else 0
        pid, pdd = self.pend[t][:P], self.pendd[t][:P]
        ln, pl = int((ids != EMPTY).sum()), int((pid != EMPTY).sum())
        k = min(len(srcs), NC)
        if flush and pl == 0:
            return
        if not flush:  # a proposal whose source the list or the pending area already holds is dropped (refine passes only)
            srcs, od = srcs[:k], od[:k]
            new = ~(np.isin(srcs, ids[:ln]) | np.isin(srcs, pid[:pl]))
            c["dup_skipped"] += k - int(new.sum())
            srcs, od = srcs[new], od[new]
            k = len(srcs)
            if k == 0:
                return
        room = cap - ln
        if not flush and k <= room + (P - pl):
            a = min(k, room)
            ids[ln: ln + a], ds[ln: ln + a] = srcs[:a], orderable_f32(od[:a])
            pid[pl: pl + k - a], pdd[pl: pl + k - a] = srcs[a:k], orderable_f32(od[a:k])
            c["appends_list"] += a
            c["appends_pend"] += k - a
            return
        if ln + pl + k > NC:
            k = NC - ln - pl
            c["runs_cut"] += 1
        key = np.sort(np.concatenate([pack(ds[:ln], ids[:ln]), pack(pdd[:pl], pid[:pl]),
                                      (od[:k].astype(np.uint64) << S32) | srcs[:k].astype(np.uint64)]))
        cid = (key & LOW).astype(np.uint32)
        cd = orderable_f32((key >> S32).astype(np.uint32))
        kept = self._prune(cid, cd, cap, alpha, True)
        ns = len(kept)
        ids[:ns], ds[:ns] = cid[kept], cd[kept]
        ids[ns:], ds[ns:] = EMPTY, 0.0
        pid[:], pdd[:] = EMPTY, 0.0
        c["flushed" if flush else "prunes_merge"] += 1
        c["prunes_upper"] += level > 0

    def _link_level(self, rows, level, keys, counts, exp, nexp, alpha):
        t_all, d_all, s_all = [], [], []
        for i, q in enumerate(rows):
            sid, sd = self._select(int(q), level, keys[i], counts[i], None if exp is None else exp[i], None if exp is None else nexp[i], alpha)
            t_all.append(sid)
            d_all.append(f32_orderable(sd))
            s_all.append(np.full(len(sid), q, np.uint32))
        tgt, od, src = np.concatenate(t_all), np.concatenate(d_all), np.concatenate(s_all)
        if not len(tgt):
            return
        pk = (tgt.astype(np.uint64) << S32) | od.astype(np.uint64)
        o = np.argsort(pk, kind="stable")  # the radix sort is stable: equal (target, dist) keep batch order
        pk, tgt, od, src = pk[o], tgt[o], od[o], src[o]
        self.c["ties"] += int((pk[1:] == pk[:-1]).sum())
        heads = np.flatnonzero(np.concatenate([[True], tgt[1:] != tgt[:-1]]))
        ends = np.concatenate([heads[1:], [len(tgt)]])
        for a, b in zip(heads, ends):
            self._merge(int(tgt[a]), level, src[a:b], od[a:b], alpha)

    # ---- builder_insert_range ----------------------------------------------------------------------
    def _insert_range(self, s0, n, alpha, refine=False):
        po, efc = self.po, self.efc
        algo = 0 if self.hnsw else 1
        s = s0
        for B in batch_sizes(s0, n, self.fraction, refine):
            batch = self.order[s: s + B]
            G = po.Graph.from_arrays(self.X, self.M, self.M0, self.max_level, self.entry, self.levels, self.upper_off, self.adj0, self.adjU)
            jobs = []
            if self.leveled:
                for l in range(self.max_level, 0, -1):
                    rows = batch[self.levels[batch] >= l]
                    if len(rows):
                        keys, counts, _, _ = G.search_level_batch(rows, l, efc, algo, 0, self.nthreads)
                        jobs.append((l, rows, keys, counts))
            keys0, counts0, exp, nexp = G.search_level_batch(batch, 0, efc, algo, 0 if self.hnsw else EXPCAP, self.nthreads)
            del G  # every search of the batch is done before the first list changes
            for l, rows, keys, counts in jobs:
                self._link_level(rows, l, keys, counts, None, None, alpha)
            self._link_level(batch, 0, keys0, counts0, None if self.hnsw else exp, nexp, alpha)
            if self.leveled:
                for q in batch:
                    if self.levels[q] > self.max_level:
                        self.max_level, self.entry = int(self.levels[q]), int(q)
            s += B
            self.batches.append(B)

    def _finish(self):
        if self.P and self.n:
            for t in range(self.n):
                self._merge(t, 0, np.zeros(0, np.uint32), np.zeros(0, np.uint32), self.alpha, flush=True)
        return self.graph()

    def build(self):
        n = self.n
        alpha = np.float32(0.0) if self.hnsw else self.alpha
        if n == 0:
            return self.graph()
        if self.leveled:
            self.order = insertion_order(0, n)
            first = int(self.order[0])
        else:
            first, self.medoid_gap = medoid(self.X)
            self.order = insertion_order(0, n, first)
        self.entry, self.max_level = first, int(self.levels[first])
        if self.passes > 1 and not self.hnsw:
            alpha = self.alpha1
        self._insert_range(1, n, alpha)
        for p in range(1, self.passes):
            if self.hnsw or n <= 1:
                break
            if p == self.passes - 1:
                alpha = self.alpha
            self._insert_range(0, n, alpha, refine=True)
        return self._finish()

    def continue_from(self, g, n_old):
        """append (leann_backend_add): rows [n_old, n) continue the batched insertion from graph g over rows [0, n_old); the stored
        link distances are recomputed from the rows, as link_dist_kernel does"""
        assert self.hnsw and (g["levels"][:n_old] == self.levels[:n_old]).all()
        old_lists = int(self.levels[:n_old].astype(np.int64).sum())
        self.adj0[:n_old] = g["adj0"][:n_old]
        self.adjU[:old_lists] = g["adjU"][:old_lists]
        X64 = self.X.astype(np.float64)
        for i in range(n_old):
            for level in range(int(self.levels[i]) + 1):
                ids, ds = self._list(i, level)
                m = ids != EMPTY
                ds[m] = (np.float32(1.0) - (X64[ids[m]] @ X64[i]).astype(np.float32)).astype(np.float32)
        self.entry, self.max_level = int(g["entry"]), int(g["max_level"])
        self.order = insertion_order(n_old, self.n)
        self._insert_range(n_old, self.n, np.float32(0.0))
        return self._finish()

    def graph(self):
        return dict(kind=self.kind, X=self.X, M=self.M, M0=self.M0, max_level=self.max_level, entry=self.entry, levels=self.levels,
                    upper_off=self.upper_off[: self.n], adj0=self.adj0[: self.n], adjU=self.adjU[: self.nu], counters=dict(self.c),
                    batches=list(self.batches))


def check_lists(g):
    """ids < n, compact, no self loop, no duplicate, degree <= width, on every level; -> list of complaints"""
    bad, n = [], len(g["levels"])
    for name, A, owner in (("adj0", g["adj0"], np.arange(n)),
                           ("adjU", g["adjU"], np.repeat(np.arange(n), g["levels"].astype(np.int64)))):
        if A.size == 0:
            continue
        v = A != EMPTY
        if (A[v] >= n).any():
            bad.append(f"{name}: id >= n")
        if not (v[:, :-1] >= v[:, 1:]).all():
            bad.append(f"{name}: list not compact")
        if (A == owner[:, None]).any():
            bad.append(f"{name}: self loop at {np.flatnonzero((A == owner[:, None]).any(1))[:5].tolist()}")
        s = np.sort(A, axis=1)
        dup = ((s[:, 1:] == s[:, :-1]) & (s[:, 1:] != EMPTY)).any(1)
        if dup.any():
            bad.append(f"{name}: duplicate id in {int(dup.sum())} lists, first {np.flatnonzero(dup)[:5].tolist()}")
    return bad


# The cases of tests/test_gpu_build_parity.py (and of test_cpu_build_ref.py, which checks the restatement alone): `need` = the
# counters that must be non-zero for the case to exercise what it is there for; `zero` = counters that must stay zero.
HN, VA = "hnsw", "diskann"
_V = dict(kind=VA, n=1500, d=128, M=24, efc=48, shape="blocks", seed=5)
CASES = {
    "hnsw_m8": dict(kind=HN, n=1200, d=40, M=8, efc=48, need=("appends_list", "prunes_merge", "prunes_upper", "pools_33_64", "ties")),
    "hnsw_m4_d768": dict(kind=HN, n=600, d=768, M=4, efc=24, need=("pools_le32", "prunes_merge")),
    "hnsw_efc160": dict(kind=HN, n=1000, d=38, M=8, efc=160, need=("pools_gt64", "pools_cut_nc", "prunes_merge")),
    "hnsw_m48_wide": dict(kind=HN, n=1500, d=64, M=48, efc=200, shape="hubs", need=("kept_gt64", "pools_gt176", "prunes_merge")),
    "hnsw_fraction_1": dict(kind=HN, n=400, d=40, M=8, efc=48, knobs={"LEANN_BUILD_BATCH_FRACTION": "1"}, need=("prunes_merge", "ties")),
    "hnsw_fraction_max": dict(kind=HN, n=400, d=40, M=8, efc=48, knobs={"LEANN_BUILD_BATCH_FRACTION": "1048576"}, need=("prunes_merge",)),
    "vamana_r24": dict(_V, need=("appends_list", "appends_pend", "prunes_merge", "path_taken", "path_over_max", "flushed", "ties")),
    "vamana_one_stage": dict(_V, knobs={"LEANN_VAMANA_TWO_STAGE": "0"}, need=("prunes_merge", "path_taken", "flushed")),
    "vamana_pending_0": dict(_V, knobs={"LEANN_VAMANA_PENDING": "0"}, need=("prunes_merge",), zero=("appends_pend", "flushed")),
    "vamana_pending_16": dict(_V, knobs={"LEANN_VAMANA_PENDING": "16"}, need=("appends_pend", "prunes_merge", "flushed")),
    "vamana_two_pass": dict(_V, n=800, shape="hubs", seed=1010, knobs={"LEANN_VAMANA_PASSES": "2", "LEANN_VAMANA_ALPHA1_PCT": "100"},
                            need=("self_removed", "tail_cleared", "prunes_merge", "dup_skipped")),
    "vamana_nav": dict(_V, knobs={"LEANN_VAMANA_NAV": "1"}, need=("prunes_upper", "prunes_merge", "path_taken", "flushed")),
    # a beam wider than the pool: the cut leaves 72 expanded beam entries beyond the pool's worst key, so EVERY point has more path
    # nodes than PATHMAX, and they are near candidates that the prune keeps (on the blocks rows they sit on the distance-1 plateau)
    "vamana_l200_path": dict(kind=VA, n=800, d=64, M=24, efc=200, shape="hubs", seed=11, need=("path_over_max", "path_taken", "pools_cut_nc", "prunes_merge")),
    "vamana_r96_wide": dict(kind=VA, n=1500, d=64, M=96, efc=128, shape="hubs", need=("kept_gt64", "prunes_merge", "path_taken", "appends_pend")),
}
for _i, _c in enumerate(CASES.values()):
    _c.setdefault("knobs", {})
    _c.setdefault("zero", ())
    _c.setdefault("seed", 1000 + _i)
    _c.setdefault("shape", "uniform")


def case_rows(c, n=None):
    return grid_rows(c["seed"], n or c["n"], c["d"], c["shape"])


_MEMO = {}


def case_graph(po, name):
    """the restatement's graph of a case, computed once per process and left unchanged"""
    if name not in _MEMO:
        c = CASES[name]
        _MEMO[name] = BuildRef(po, c["kind"], case_rows(c), c["M"], c["efc"], c["knobs"]).build()
    return _MEMO[name]
