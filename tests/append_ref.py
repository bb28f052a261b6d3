"""leann_backend_append restated from its definition (include/leann_backend.h "appending to a handle") on top of build_ref.BuildRef,
for tests/test_gpu_append.py.

BuildRef.continue_from restates the file twin (leann_backend_add): HNSW only, and the old levels must be the builder's hash.  An
append to a HANDLE also continues a Vamana graph and a graph whose levels are not the hash (from_arrays, a compaction), so this
subclass takes the old graph as it is:

  levels     positions < n_old keep the old graph's, positions >= n_old get the hash (Vamana: 0); upper_off = the exclusive prefix sum
  lists      the old level-0 lists and the old upper lists, in place; stored distances recomputed from the rows; pending area empty
  start      the old entry and max_level (Vamana: the old medoid, not recomputed)
  insertion  insertion_order(n_old, n), batch_sizes(n_old, ..) under LEANN_BUILD_BATCH_FRACTION, no refine passes; HNSW prunes with
             alpha 0 (the heuristic), Vamana with alpha 1.2 and the prune form the OLD graph was built with (`two_stage`)
  finish     whatever is pending is folded into its list, over all n positions"""
import numpy as np

import build_ref as br


class AppendRef(br.BuildRef):
    def __init__(self, po, kind, X, M, efc, old, two_stage=True, knobs=None):
        """X: all n rows, the old graph's first; old: dict with levels, upper_off, adj0, adjU, entry, max_level over X[:n_old]"""
        knobs = dict(knobs or {})
        knobs["LEANN_VAMANA_TWO_STAGE"] = "1" if two_stage else "0"   # the form the handle recorded, not the environment's
        knobs.pop("LEANN_VAMANA_PASSES", None)
        knobs.pop("LEANN_VAMANA_NAV", None)
        super().__init__(po, kind, X, M, efc, knobs)
        self.old = old
        self.n_old = n_old = len(old["levels"])
        assert n_old <= self.n
        self.levels[:n_old] = old["levels"]
        assert (np.asarray(old["upper_off"], np.int64)
                == np.concatenate([[0], np.cumsum(np.asarray(old["levels"], np.int64))[:-1]])[:n_old]).all()
        self.upper_off[:] = 0
        self.upper_off[1: self.n] = np.cumsum(self.levels.astype(np.uint64))[:-1]
        self.nu = int(self.levels.astype(np.int64).sum())
        self.adjU = np.full((max(self.nu, 1), M), br.EMPTY, np.uint32)
        self.adjdU = np.zeros((max(self.nu, 1), M), np.float32)

    def run(self):
        old, n_old = self.old, self.n_old
        old_lists = int(self.levels[:n_old].astype(np.int64).sum())
        self.adj0[:n_old] = old["adj0"][:n_old]
        self.adjU[:old_lists] = old["adjU"][:old_lists]
        X64 = self.X.astype(np.float64)
        for i in range(n_old):  # link_dist_kernel: exact on the grid rows in any summation order
            for level in range(int(self.levels[i]) + 1):
                ids, ds = self._list(i, level)
                m = ids != br.EMPTY
                ds[m] = (np.float32(1.0) - (X64[ids[m]] @ X64[i]).astype(np.float32)).astype(np.float32)
        self.entry, self.max_level = int(old["entry"]), int(old["max_level"])
        self.order = br.insertion_order(n_old, self.n)
        self._insert_range(n_old, self.n, np.float32(0.0) if self.hnsw else self.alpha)
        return self._finish()
