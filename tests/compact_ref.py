"""Compaction (DESIGN.md §5b "Compaction") restated in plain numpy, for tests/test_cpu_compact.py and tests/test_gpu_compact.py.

compact(g, removed) -> (g', new_to_old) on the graph dict of consolidate_ref.py.  With p_0 < p_1 < ... the live positions:
    X, levels     row / level of p_j at j
    adj0          the level-0 list of p_j at j, slot for slot, ids mapped old -> new (EMPTY slots stay where they are)
    adjU          the upper lists of p_j, in level order, at upper_off'[j] ..., mapped the same way
    upper_off     the exclusive prefix sum of the gathered levels
    entry         map(entry);  kind, M, M0, max_level unchanged
new_to_old [live] int64 = p.  The input must be consolidated: a live list that names a removed id, or a removed entry, asserts."""
import numpy as np

EMPTY = 0xFFFFFFFF


def _remap(lists, old_to_new):
    """ids of `lists` through old_to_new, EMPTY slots kept; no live id may map to EMPTY"""
    out = np.full(lists.shape, EMPTY, np.uint32)
    named = lists != EMPTY
    out[named] = old_to_new[lists[named].astype(np.int64)]
    assert not (out[named] == EMPTY).any(), "a live list names a removed id: consolidate first"
    return out


def compact(g, removed):
    removed = np.asarray(removed, bool)
    n = len(removed)
    assert n == len(g["X"]) == len(g["levels"]) and not removed.all()
    new_to_old = np.flatnonzero(~removed)
    live = len(new_to_old)
    old_to_new = np.full(n, EMPTY, np.uint32)
    old_to_new[new_to_old] = np.arange(live, dtype=np.uint32)
    assert not removed[g["entry"]], "the entry point is removed: consolidate first"
    levels = g["levels"][new_to_old]
    upper_off = np.zeros(live, np.uint32)
    upper_off[1:] = np.cumsum(levels.astype(np.uint32))[:-1]
    # the upper lists of a node are the run upper_off[v] .. upper_off[v] + levels[v] - 1
    rows = [int(g["upper_off"][p]) + l for p, lv in zip(new_to_old, levels) for l in range(int(lv))]
    adjU = g["adjU"][np.asarray(rows, np.int64)] if rows else g["adjU"][:0]
    out = dict(g)
    out.pop("counters", None)
    out.pop("counters_by_level", None)
    out.update(X=g["X"][new_to_old], levels=levels, upper_off=upper_off, adj0=_remap(g["adj0"][new_to_old], old_to_new),
               adjU=_remap(adjU, old_to_new), entry=int(old_to_new[g["entry"]]))
    return out, new_to_old
