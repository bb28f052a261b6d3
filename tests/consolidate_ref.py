"""Delete consolidation restated in plain numpy, for tests/test_gpu_delete.py, tests/test_gpu_delete_edges.py and
tests/test_cpu_delete.py.

A graph is a dict: kind ("hnsw" | "diskann"), X [n x d] f32, M, M0, max_level, entry, levels [n] u8, upper_off [n] u32,
adj0 [n x M0] u32, adjU [n_upper_lists x M] u32 (EMPTY-padded lists; the list of node v on level l >= 1 is adjU[upper_off[v] + l - 1]).

Per level, for every live node p whose list names a removed id:
    C = (N(p) \\ D)  u  U_{v in N(p) & D} (N(v) \\ D),  p excluded, N(.) read from the graph as it was before the pass;
    dist(p, c) = 1 - <x_p, x_c> in f32; candidates sorted by (dist, id), equal ids dropped, the NC nearest kept
    (NC = 128, or 256 when a list holds more than 64 ids); then the builder's prune rule with the list width as the limit:
    HNSW (alpha = 0): walk the candidates in order, drop c if some kept k has dist(c, k) < dist(c, p);
    Vamana one-stage: drop c if alpha * dist(c, k) <= dist(c, p);
    Vamana two-stage (alpha > 1): a first walk with alpha = 1 over the whole pool, then the free slots are filled from the
    candidates it passed over by the relaxed rule.
Lists of removed nodes are cleared; a removed entry point is replaced (HNSW / leveled: the live node of the highest level, lowest
id on ties, max_level following it down; single-level DiskANN: the live row nearest to the old entry's row, lower id on ties).
The distances are exact f32 only for inputs whose dot products are exact in f32 (the tests' rows are multiples of 1/8).

Two row recipes (random_graph(rows=...)).  "dense": every coordinate drawn from {-2..2}/8; two random rows are then never
orthogonal, the prune rule drops nearly every candidate and no repaired list passes ~44 ids.  "sparse": `nnz` non-zero coordinates
per row, drawn from {-2, -1, 1, 2}/8; most pairs are orthogonal (distance exactly 1.0, ordered by id), which the HNSW rule (strict <)
and Vamana's second stage keep, so repaired lists come out full.  "mixed": every dense_every-th row dense, the others sparse.  A
kept dense row occludes about half of the sparse rows behind it, so half and half is as short as dense; one dense row in 40 gives
lengths on both sides of 64.
Either way |x| <= 2/8 and every product is a multiple of 1/64: at d = 4096 a dot product stays below 256 in magnitude, so it and
1 - dot are exact in f32 in any summation order.

consolidate() also counts which paths of the repair ran (out["counters"], out["counters_by_level"]; COUNTERS below), so that a test
case can state the branch it exists for and tests/test_cpu_delete.py can hold it to that without a device."""
import numpy as np

EMPTY = 0xFFFFFFFF

# repairs              live nodes whose list named a removed id (one workgroup each)
# pools_*              size of the candidate pool handed to the prune, after the cut at NC: 0, 1, 2..32, 33..64, 65..128, 129..255;
#                      pools_eq_nc: exactly NC (128 counts in pools_65_128 too); pools_cut: more than NC unique candidates existed
# lists_gt64           repaired lists longer than 64; lists_gt64_not_full: of those, shorter than the width; lists_full: == width
# all_removed          repaired nodes whose list named removed ids only; all_removed_full: ... and held `width` of them
# empty_chunks         NC-sized chunks of the slot sequence (the node's own list, then its removed neighbours' lists in list order,
#                      each `width` slots) in which nothing is live; dup_chunks: chunks that bring an id the running best-NC holds
# second_stage_keeps   ids taken by the relaxed second walk of the two-stage Vamana rule
COUNTERS = ("repairs", "pools_0", "pools_1", "pools_2_32", "pools_33_64", "pools_65_128", "pools_129_255", "pools_eq_nc", "pools_cut",
            "lists_gt64", "lists_gt64_not_full", "lists_full", "all_removed", "all_removed_full", "empty_chunks", "dup_chunks",
            "second_stage_keeps")


def pool_size(g):
    return 256 if max(g["M"], g["M0"]) > 64 else 128


def _dist(X, p, ids):
    dot = (X[ids].astype(np.float64) @ X[p].astype(np.float64)).astype(np.float32)
    return (np.float32(1.0) - dot).astype(np.float32)


def candidates(g, removed, level, p, old, info=None):
    """ids and distances of the pool of node p on `level`, ascending by (dist, id), unique, at most NC.  `old(v)` = N(v) on that level.
    info["unique"] = the number of unique candidates before the cut."""
    own = old(p)
    own = own[own != EMPTY]
    parts = [own[~removed[own]]]
    for v in own[removed[own]]:
        nv = old(int(v))
        nv = nv[nv != EMPTY]
        parts.append(nv[~removed[nv]])
    c = np.unique(np.concatenate(parts)) if parts else np.zeros(0, np.uint32)
    c = c[c != p].astype(np.int64)
    if info is not None:
        info["unique"] = int(c.size)
    if c.size == 0:
        return c, np.zeros(0, np.float32)
    d = _dist(g["X"], p, c)
    order = np.lexsort((c, d))[: pool_size(g)]
    return c[order], d[order]


def prune(X, cid, cd, limit, alpha, two_stage, info=None):
    """positions (into cid) kept by the builder's prune_core, in kept order; info["second_stage"] = how many the second walk took"""
    if info is not None:
        info["second_stage"] = 0
    nc = len(cid)
    if nc == 0:
        return []
    Xc = X[cid].astype(np.float64)
    G = (np.float32(1.0) - (Xc @ Xc.T).astype(np.float32)).astype(np.float32)
    alpha = np.float32(alpha)
    ts = bool(alpha > 1.0 and two_stage)
    a1 = np.float32(1.0) if ts else alpha
    kept, taken = [], np.zeros(nc, bool)
    for i in range(nc):
        if kept:
            gk = G[i, kept]
            bad = (gk < cd[i]).any() if alpha == 0 else ((a1 * gk).astype(np.float32) <= cd[i]).any()
            if bad:
                continue
        kept.append(i)
        taken[i] = True
        if len(kept) == limit:
            return kept
    if ts:
        for i in range(nc):
            if taken[i]:
                continue
            if ((alpha * G[i, kept]).astype(np.float32) <= cd[i]).any():
                continue
            kept.append(i)
            if info is not None:
                info["second_stage"] += 1
            if len(kept) == limit:
                break
    return kept


def chunk_walk(g, removed, p, own, old, W, NC):
    """the repair kernel's chunked read of the pool, restated for the counters: slots = own list, then the lists of its removed
    neighbours in list order; chunks of NC slots merged into a running best-NC by (dist, id).
    -> (chunks without a live id, chunks that bring an id the running best already holds, ids of the final best)"""
    dead = [int(v) for v in own if v != EMPTY and removed[v]]
    slots = np.concatenate([own] + [old(v) for v in dead]).astype(np.int64)
    ok = (slots != EMPTY) & (slots != p)
    ok[ok] = ~removed[slots[ok]]
    ids = np.unique(slots[ok])
    dist = dict(zip(ids.tolist(), _dist(g["X"], p, ids).tolist())) if ids.size else {}
    best = np.zeros(0, np.int64)
    empty = dup = 0
    for c0 in range(0, len(slots), NC):
        c = np.unique(slots[c0: c0 + NC][ok[c0: c0 + NC]])
        if c.size == 0:
            empty += 1
            continue
        dup += bool(np.intersect1d(c, best).size)
        u = np.union1d(c, best)
        d = np.array([dist[int(i)] for i in u], np.float32)
        best = u[np.lexsort((u, d))[:NC]]
    return empty, dup, best


def consolidate(g, removed, alpha=1.2, two_stage=True):
    """-> a new graph dict with adj0 / adjU / entry / max_level after the repair, plus "counters" (totals) and "counters_by_level";
    the input is not modified"""
    removed = np.asarray(removed, bool)
    n = len(removed)
    out = dict(g)
    NC = pool_size(g)
    by_level = [dict.fromkeys(COUNTERS, 0) for _ in range(g["max_level"] + 1)]
    out["adj0"] = g["adj0"].copy()
    out["adjU"] = g["adjU"].copy()
    levels = g["levels"]
    hnsw = g["kind"] == "hnsw"
    a = 0.0 if hnsw else alpha
    for level in range(g["max_level"] + 1):
        W = g["M0"] if level == 0 else g["M"]
        src = g["adj0"] if level == 0 else g["adjU"]
        dst = out["adj0"] if level == 0 else out["adjU"]

        def row(v, level=level):
            return v if level == 0 else int(g["upper_off"][v]) + level - 1

        def old(v, src=src):
            return src[row(v)]

        for p in range(n):
            if levels[p] < level:
                continue
            if removed[p]:
                dst[row(p)] = EMPTY
                continue
            l = old(p)
            l = l[l != EMPTY]
            if not removed[l].any():
                continue
            info = {}
            cid, cd = candidates(g, removed, level, p, old, info)
            kept = prune(g["X"], cid, cd, W, a, two_stage, info)
            empty, dup, best = chunk_walk(g, removed, p, old(p), old, W, NC)
            assert (np.sort(best) == np.sort(cid)).all()         # the chunked running best is the global best-NC
            cn, nc = by_level[level], len(cid)
            cn["repairs"] += 1
            size = ("pools_0" if nc == 0 else "pools_1" if nc == 1 else "pools_2_32" if nc <= 32 else "pools_33_64" if nc <= 64 else
                    "pools_65_128" if nc <= 128 else "pools_129_255" if nc <= 255 else None)
            if size:
                cn[size] += 1
            cn["pools_eq_nc"] += nc == NC
            cn["pools_cut"] += info["unique"] > NC
            cn["lists_gt64"] += len(kept) > 64
            cn["lists_gt64_not_full"] += 64 < len(kept) < W
            cn["lists_full"] += len(kept) == W
            cn["all_removed"] += bool(removed[l].all())
            cn["all_removed_full"] += bool(removed[l].all() and len(l) == W)
            cn["empty_chunks"] += empty
            cn["dup_chunks"] += dup
            cn["second_stage_keeps"] += info["second_stage"]
            new = np.full(W, EMPTY, np.uint32)
            new[: len(kept)] = cid[kept]
            dst[row(p)] = new
    e = int(g["entry"])
    live = np.flatnonzero(~removed)
    if removed[e] and live.size:
        if g["max_level"] == 0 and not hnsw:
            d = _dist(g["X"], e, live)
            out["entry"] = int(live[np.lexsort((live, d))[0]])
        else:
            top = int(levels[live].max())
            out["entry"] = int(live[levels[live] == top][0])
            out["max_level"] = min(g["max_level"], top)
    out["counters_by_level"] = [{k: int(v) for k, v in cn.items()} for cn in by_level]
    out["counters"] = {k: sum(cn[k] for cn in out["counters_by_level"]) for k in COUNTERS}
    return out


def pending(g, removed):
    """number of removed positions that a live node's list (any level) still names"""
    removed = np.asarray(removed, bool)
    named = np.zeros(len(removed), bool)
    for level in range(g["max_level"] + 1):
        for p in np.flatnonzero(~removed & (g["levels"] >= level)):
            l = g["adj0"][p] if level == 0 else g["adjU"][int(g["upper_off"][p]) + level - 1]
            l = l[l != EMPTY]
            named[l[removed[l]]] = True
    return int(named.sum())


def sparse_rows(rng, n, d, nnz):
    """`nnz` non-zero coordinates per row, each from {-2, -1, 1, 2}/8, at random places"""
    X = np.zeros((n, d), np.float32)
    vals = np.array([-2, -1, 1, 2], np.float32) / np.float32(8)
    for i in range(n):
        X[i, rng.choice(d, nnz, replace=False)] = vals[rng.integers(0, 4, nnz)]
    return X


def random_graph(rng, kind, n, d, M, M0, max_level, rows="dense", nnz=8, dense_every=2):
    """rows with coordinates in {-2..2}/8 (every dot product and 1 - dot exact in f32 in any summation order) and random lists;
    rows: "dense" | "sparse" | "mixed" (every dense_every-th row dense, the others sparse), see the module docstring"""
    X = (rng.integers(-2, 3, (n, d)) / 8.0).astype(np.float32)
    if rows != "dense":
        S = sparse_rows(rng, n, d, nnz)
        if rows == "mixed":
            S[0::dense_every] = X[0::dense_every]
        X = S
    levels = np.zeros(n, np.uint8)
    if max_level:
        levels = np.minimum(rng.geometric(0.75, n) - 1, max_level).astype(np.uint8)
        levels[int(rng.integers(n))] = max_level
    upper_off = np.zeros(n, np.uint32)
    upper_off[1:] = np.cumsum(levels.astype(np.uint32))[:-1]
    n_upper = int(levels.astype(np.int64).sum())
    adj0 = np.full((n, M0), EMPTY, np.uint32)
    adjU = np.full((max(n_upper, 1), M), EMPTY, np.uint32)
    for level in range(max_level + 1):
        W = M0 if level == 0 else M
        members = np.flatnonzero(levels >= level)
        for p in members:
            others = members[members != p]
            k = min(int(rng.integers(W // 2, W + 1)), len(others))
            l = rng.choice(others, k, replace=False).astype(np.uint32)
            if level == 0:
                adj0[p, :k] = l
            else:
                adjU[int(upper_off[p]) + level - 1, :k] = l
    entry = int(np.flatnonzero(levels == levels.max())[0])
    return dict(kind=kind, X=X, M=M, M0=M0, max_level=int(levels.max()), entry=entry, levels=levels, upper_off=upper_off,
                adj0=adj0, adjU=adjU[:n_upper] if n_upper else adjU[:0])
