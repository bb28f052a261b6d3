"""Delete consolidation restated in plain numpy, for tests/test_gpu_delete.py and tests/test_cpu_delete.py.

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
The distances are exact f32 only for inputs whose dot products are exact in f32 (the tests' rows are multiples of 1/8)."""
import numpy as np

EMPTY = 0xFFFFFFFF


def pool_size(g):
    return 256 if max(g["M"], g["M0"]) > 64 else 128


def _dist(X, p, ids):
    dot = (X[ids].astype(np.float64) @ X[p].astype(np.float64)).astype(np.float32)
    return (np.float32(1.0) - dot).astype(np.float32)


def candidates(g, removed, level, p, old):
    """ids and distances of the pool of node p on `level`, ascending by (dist, id), unique, at most NC.  `old(v)` = N(v) on that level."""
    own = old(p)
    own = own[own != EMPTY]
    parts = [own[~removed[own]]]
    for v in own[removed[own]]:
        nv = old(int(v))
        nv = nv[nv != EMPTY]
        parts.append(nv[~removed[nv]])
    c = np.unique(np.concatenate(parts)) if parts else np.zeros(0, np.uint32)
    c = c[c != p].astype(np.int64)
    if c.size == 0:
        return c, np.zeros(0, np.float32)
    d = _dist(g["X"], p, c)
    order = np.lexsort((c, d))[: pool_size(g)]
    return c[order], d[order]


def prune(X, cid, cd, limit, alpha, two_stage):
    """positions (into cid) kept by the builder's prune_core, in kept order"""
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
            if len(kept) == limit:
                break
    return kept


def consolidate(g, removed, alpha=1.2, two_stage=True):
    """-> a new graph dict with adj0 / adjU / entry / max_level after the repair; the input is not modified"""
    removed = np.asarray(removed, bool)
    n = len(removed)
    out = dict(g)
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
            cid, cd = candidates(g, removed, level, p, old)
            kept = prune(g["X"], cid, cd, W, a, two_stage)
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


def random_graph(rng, kind, n, d, M, M0, max_level):
    """rows with coordinates in {-2..2}/8 (every dot product and 1 - dot exact in f32 in any summation order) and random lists"""
    X = (rng.integers(-2, 3, (n, d)) / 8.0).astype(np.float32)
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
