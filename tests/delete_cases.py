"""The graphs of tests/test_gpu_delete_edges.py, stated once so that tests/test_cpu_delete.py can hold every case to the branch of
the repair it exists for (consolidate_ref.COUNTERS) without a device.

A case: the graph recipe (consolidate_ref.random_graph), the share of rows removed, hand-built nodes, and `need`: counter -> the
least value the reference must count ("all": as many as there are repairs).  "L<l>." in front of a counter reads the counters of
level l, "U." the sum over the levels >= 1.  n is 515 or 643: neither a multiple of 8 (tail bits of the live mask) nor of 256 (tail
of the mark / pending grids).  graph() and reference() are computed once per process and must not be modified by their callers."""
import functools

import numpy as np

import consolidate_ref as cr

EMPTY = cr.EMPTY


def _case(kind, d, M, M0, max_level, n=515, rows="dense", nnz=8, dense_every=2, frac=0.30, two_stage=True, full_dead=False,
          empty_pool=False, key_offset=0, seed=1, **need):
    return dict(kind=kind, d=d, M=M, M0=M0, max_level=max_level, n=n, rows=rows, nnz=nnz, dense_every=dense_every, frac=frac,
                two_stage=two_stage, full_dead=full_dead, empty_pool=empty_pool, key_offset=key_offset, seed=seed, need=need)


CASES = {
    # every pair of sparse rows but a few is orthogonal: nothing is pruned, level-0 lists come back with 128 ids, upper ones with 64
    "hnsw_m64": _case("hnsw", 1024, 64, 128, 2, n=643, rows="sparse", nnz=3,
                      **{"lists_gt64": 1, "L0.lists_full": 1, "U.lists_full": 1, "pools_eq_nc": 1, "U.repairs": 1}),
    # half dense, half sparse does not get there: a sparse node's nearest candidates are then dense rows, and every kept dense row
    # occludes about half of the sparse ones behind it (no list passes 48).  One dense row in 40 among rows of 3 non-zeros in 256
    # coordinates does: level-0 lists from under 16 to over 96 ids, some of exactly 64
    "hnsw_m64_mixed": _case("hnsw", 256, 64, 128, 2, n=643, rows="mixed", nnz=3, dense_every=40,
                            **{"lists_gt64_not_full": 1, "U.repairs": 1}),
    "vamana_r128": _case("diskann", 256, 128, 128, 0, n=643, rows="sparse", full_dead=True,
                         lists_full=1, second_stage_keeps=1, all_removed_full=1, lists_gt64=1),
    "vamana_r128_one_stage": _case("diskann", 256, 128, 128, 0, n=643, rows="sparse", two_stage=False, full_dead=True,
                                   lists_full=1, all_removed_full=1, lists_gt64=1),
    "vamana_r64": _case("diskann", 40, 64, 64, 0, pools_eq_nc="all", repairs=1),            # the last narrow width: NC = 128
    "vamana_r65": _case("diskann", 40, 65, 65, 0, frac=0.06, pools_129_255=1, pools_eq_nc=1),  # the first wide one, no multiple of 4
    "hnsw_m8_d1536": _case("hnsw", 1536, 8, 16, 2, frac=0.15, pools_2_32=1, pools_33_64=1, pools_65_128=1),
    "vamana_r32_d4096": _case("diskann", 4096, 32, 32, 0, pools_cut=1),
    "vamana_r96_d1100": _case("diskann", 1100, 96, 96, 0, repairs=1, empty_pool=True, pools_0=1),
    "hnsw_m8_d30": _case("hnsw", 30, 8, 16, 2, repairs=1),
    "hnsw_m8_d100": _case("hnsw", 100, 8, 16, 2, key_offset=1_000_000, repairs=1),
    # most of every list removed: small pools on every level, chunks of 128 slots (8 lists of level 0) without a live id.  A pool of
    # one id does not occur at 60 % (seeds 1..7); at 90 % pools of one and of none do, on the upper levels
    "hnsw_m8_60": _case("hnsw", 40, 8, 16, 2, frac=0.60, seed=4,
                        **{"L0.pools_2_32": 1, "L1.pools_2_32": 1, "L2.pools_2_32": 1, "empty_chunks": 1}),
    "hnsw_m8_90": _case("hnsw", 40, 8, 16, 2, n=643, frac=0.90, seed=3,
                        **{"pools_1": 1, "pools_0": 1, "L0.pools_2_32": 1, "L1.pools_2_32": 1, "L2.pools_2_32": 1, "empty_chunks": 1}),
}


def counter(want, key):
    """the value of a `need` key in the counters of a consolidate_ref.consolidate result"""
    if key.startswith("U."):
        return sum(cn[key[2:]] for cn in want["counters_by_level"][1:])
    if key.startswith("L"):
        lvl, name = key[1:].split(".")
        return want["counters_by_level"][int(lvl)][name] if int(lvl) < len(want["counters_by_level"]) else 0
    return want["counters"][key]


def check_needs(name, want):
    for key, least in CASES[name]["need"].items():
        got = counter(want, key)
        least = want["counters"]["repairs"] if least == "all" else least
        assert got >= least, f"{name}: the reference counts {key} = {got}, the case needs {least}: {want['counters']}"


def clean_nodes(g, removed, k=8):
    """k live level-0 nodes whose lists are cut down to their live ids: they name nothing removed and must come back byte-identical
    (at 30 % removed a random list of 32+ ids is never clean by itself).  -> the live level-0 nodes behind them, for other hand-built nodes"""
    live = np.flatnonzero(~removed & (g["levels"] == 0))
    for c in live[:k]:
        l = g["adj0"][c]
        keep = l[(l != EMPTY) & ~removed[np.where(l == EMPTY, 0, l)]]
        g["adj0"][c] = EMPTY
        g["adj0"][c, : len(keep)] = keep
    return live[k:]


@functools.lru_cache(maxsize=None)
def graph(name):
    """-> (graph dict, removed [n] bool, dict of the hand-built nodes)"""
    c = CASES[name]
    rng = np.random.default_rng([c["seed"], len(name)])
    g = cr.random_graph(rng, c["kind"], c["n"], c["d"], c["M"], c["M0"], c["max_level"], rows=c["rows"], nnz=c["nnz"],
                        dense_every=c["dense_every"])
    removed = rng.random(c["n"]) < c["frac"]
    removed[g["entry"]] = True
    rest = clean_nodes(g, removed)
    dead = np.flatnonzero(removed)
    special = {}
    if c["full_dead"]:          # a node whose list is full and names removed ids only: s_nsrc = width + 1, the most slots there can be
        a = int(rest[0])
        g["adj0"][a] = rng.choice(dead, c["M0"], replace=False)
        special["full_dead"] = a
    if c["empty_pool"]:         # b's only neighbour is removed and names nothing live but b itself: nc == 0, the list comes back empty
        b, r = int(rest[1]), int(dead[0])
        g["adj0"][b] = EMPTY
        g["adj0"][b, 0] = r
        g["adj0"][r] = EMPTY
        g["adj0"][r, :3] = [b, dead[1], dead[2]]
        special["empty_pool"] = b
    return g, removed, special


@functools.lru_cache(maxsize=None)
def reference(name):
    g, removed, _ = graph(name)
    return cr.consolidate(g, removed, alpha=1.2, two_stage=CASES[name]["two_stage"])
