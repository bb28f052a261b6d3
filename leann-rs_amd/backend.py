"""Host-side mirror of leann-rs's backend layer (src/backend/{mod,traits,hnsw,diskann}.rs) over the
C ABI.  Same names, argument meaning and error behaviour; the arithmetic runs in HIP kernels."""
import ctypes as C
import enum
import os

import numpy as np

from . import _native as N
from ._native import LeannError, f32p, u32p, u64p, u8p


class BackendType(enum.IntEnum):
    """enum BackendType { Hnsw, DiskAnn } — src/backend/mod.rs:15-19"""
    Hnsw = 0
    DiskAnn = 1

    @classmethod
    def from_name(cls, name):
        # src/index/searcher.rs:95-99
        if name == "hnsw":
            return cls.Hnsw
        if name == "diskann":
            return cls.DiskAnn
        raise LeannError(1, f"Unknown backend: {name}")

    def load_searcher(self, index_path, dimensions, device=0):
        """BackendType::load_searcher — src/backend/mod.rs:23-45"""
        return BackendSearcher.load(self, index_path, dimensions, device)


class RowType(enum.IntEnum):
    """what the rows of a stored-vector index are (include/leann_backend.h "row types"); Features: a recompute-on index, no vectors"""
    F32 = 0
    BF16 = 1
    Features = 2
    I8 = 4


def round_bf16(x):
    """f32 -> bf16 bits (uint16), round to nearest even, NaN stays NaN: the library's own rounding, on the host"""
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros(x.shape, np.uint16)
    N.check(N.lib().leann_round_bf16(_p(x, f32p), x.size, out.ctypes.data_as(C.POINTER(C.c_uint16))))
    return out


def quantize_i8(x):
    """f32 rows [n x d] -> (exps int8 [d], codes int8 [n x d]): one power-of-two scale per column, codes round to nearest even and
    clamp to +-127 (include/leann_backend.h "row types"): the library's own reference quantiser, on the host"""
    x = np.ascontiguousarray(x, np.float32)
    if x.ndim != 2:
        raise LeannError(1, "quantize_i8: rows must be [n x d]")
    exps, codes = np.zeros(x.shape[1], np.int8), np.zeros(x.shape, np.int8)
    i8p = C.POINTER(C.c_int8)
    N.check(N.lib().leann_quantize_i8(_p(x, f32p), x.shape[0], x.shape[1], exps.ctypes.data_as(i8p), codes.ctypes.data_as(i8p)))
    return exps, codes


def _p(a, t):
    return a.ctypes.data_as(t) if a is not None else None


class BackendSearcher:
    """trait BackendSearcher — src/backend/traits.rs:11-30 (HnswSearcher / DiskAnnSearcher)."""

    def __init__(self, handle, backend_type):
        self._h = handle
        self.backend_type = BackendType(backend_type)

    # -- constructors -------------------------------------------------------------------------
    @classmethod
    def load(cls, backend_type, index_path, dimensions, device=0):
        """HnswSearcher::load (hnsw.rs:18-75) / DiskAnnSearcher::load (diskann.rs:21-43).  `device`: an ordinal, or a list / range
        ("0,1,2,3", "0-7") for a sharded index behind the same handle."""
        h = C.c_void_p()
        N.check(N.lib().leann_backend_open(os.fsencode(str(index_path)), int(backend_type), dimensions,
                                           str(device).encode(), C.byref(h)))
        return cls(h, backend_type)

    @classmethod
    def from_arrays(cls, backend_type, vectors, M, M0, max_level, entry, levels, upper_off, adj0, adjU,
                    device=0, key_offset=0, row_type=RowType.F32):
        vectors = np.ascontiguousarray(vectors, np.float32)
        levels = np.ascontiguousarray(levels, np.uint8)
        upper_off = np.ascontiguousarray(upper_off, np.uint32)
        adj0 = np.ascontiguousarray(adj0, np.uint32)
        adjU = np.ascontiguousarray(adjU, np.uint32)
        nul = adjU.size // M if adjU.size else 0
        h = C.c_void_p()
        n, d = vectors.shape
        if int(row_type) != RowType.F32:  # the rows are rounded on the device: the index is the f32 index over the rounded rows
            N.check(N.lib().leann_backend_from_arrays_rows(
                int(backend_type), _p(vectors, f32p), n, d, M, M0, max_level, entry, _p(levels, u8p),
                _p(upper_off, u32p), _p(adj0, u32p), _p(adjU, u32p) if nul else None, nul, device,
                key_offset, int(row_type), C.byref(h)))
            return cls(h, backend_type)
        N.check(N.lib().leann_backend_from_arrays(
            int(backend_type), _p(vectors, f32p), n, d, M, M0, max_level, entry, _p(levels, u8p),
            _p(upper_off, u32p), _p(adj0, u32p), _p(adjU, u32p) if nul else None, nul, device,
            key_offset, C.byref(h)))
        return cls(h, backend_type)

    @classmethod
    def build_device(cls, backend_type, d_vectors_ptr, n, dims, ld, graph_degree, complexity, device=0,
                     key_offset=0, take_copy=False, row_type=RowType.F32, may_overwrite=False):
        """Index straight from rows already in HBM (additive API).  row_type=RowType.BF16: the rows are rounded, the graph is built on
        the rounded rows and the handle keeps bf16 rows only; may_overwrite lets the rounding happen in the caller's buffer."""
        h = C.c_void_p()
        if int(row_type) != RowType.F32:
            N.check(N.lib().leann_backend_build_device_rows(int(backend_type), d_vectors_ptr, n, dims, ld, graph_degree, complexity,
                                                            device, key_offset, int(row_type), 1 if may_overwrite else 0, C.byref(h)))
            return cls(h, backend_type)
        N.check(N.lib().leann_backend_build_device(int(backend_type), d_vectors_ptr, n, dims, ld,
                                                   graph_degree, complexity, device, key_offset,
                                                   1 if take_copy else 0, C.byref(h)))
        return cls(h, backend_type)

    # -- trait surface ------------------------------------------------------------------------
    def search(self, query, top_k, complexity):
        """fn search(&self, query, top_k, complexity) -> (Vec<u64>, Vec<f32>) — traits.rs:16-21"""
        q = np.ascontiguousarray(query, np.float32).reshape(-1)
        if q.shape[0] != self.dims():
            raise LeannError(1, f"query has {q.shape[0]} dimensions, index has {self.dims()}")
        keys = np.zeros(max(top_k, 1), np.uint64)
        dists = np.zeros(max(top_k, 1), np.float32)
        n = C.c_size_t(0)
        N.check(N.lib().leann_backend_search(self._h, _p(q, f32p), top_k, complexity, _p(keys, u64p),
                                             _p(dists, f32p), C.byref(n)))
        return keys[: n.value].copy(), dists[: n.value].copy()

    def search_batch(self, queries, top_k, complexity):
        Q = np.ascontiguousarray(queries, np.float32)
        if Q.ndim != 2 or Q.shape[1] != self.dims():
            raise LeannError(1, f"queries must be [nq x {self.dims()}]")
        nq = Q.shape[0]
        keys = np.full((nq, top_k), np.iinfo(np.uint64).max, np.uint64)
        dists = np.full((nq, top_k), np.inf, np.float32)
        counts = np.zeros(nq, np.uint32)
        N.check(N.lib().leann_backend_search_batch(self._h, _p(Q, f32p), nq, top_k, complexity,
                                                   _p(keys, u64p), _p(dists, f32p), _p(counts, u32p)))
        return keys, dists, counts

    def search_filtered(self, query, top_k, complexity, allow):
        """search restricted to the positions whose bit is set in `allow` (uint8 bitmap, ceil(len/8) bytes);
        the filter runs inside the traversal (replaces searcher.rs:129-133 over-fetch)."""
        q = np.ascontiguousarray(query, np.float32).reshape(-1)
        if q.shape[0] != self.dims():
            raise LeannError(1, f"query has {q.shape[0]} dimensions, index has {self.dims()}")
        allow = np.ascontiguousarray(allow, np.uint8).reshape(-1)
        if allow.shape[0] < (self.len() + 7) // 8:
            raise LeannError(1, f"allow-bitmap has {allow.shape[0]} bytes, index needs {(self.len() + 7) // 8}")
        keys = np.zeros(max(top_k, 1), np.uint64)
        dists = np.zeros(max(top_k, 1), np.float32)
        n = C.c_size_t(0)
        N.check(N.lib().leann_backend_search_filtered(self._h, _p(q, f32p), top_k, complexity, _p(allow, u8p),
                                                      _p(keys, u64p), _p(dists, f32p), C.byref(n)))
        return keys[: n.value].copy(), dists[: n.value].copy()

    def search_filtered_batch(self, queries, top_k, complexity, allow):
        """allow: [ceil(len/8)] shared bitmap or [nq, stride] one bitmap per query"""
        Q = np.ascontiguousarray(queries, np.float32)
        if Q.ndim != 2 or Q.shape[1] != self.dims():
            raise LeannError(1, f"queries must be [nq x {self.dims()}]")
        allow = np.ascontiguousarray(allow, np.uint8)
        stride = 0 if allow.ndim == 1 else allow.shape[1]
        if allow.shape[-1] < (self.len() + 7) // 8 or (allow.ndim == 2 and allow.shape[0] != Q.shape[0]):
            raise LeannError(1, "allow-bitmap shape does not match the index / the batch")
        nq = Q.shape[0]
        keys = np.full((nq, top_k), np.iinfo(np.uint64).max, np.uint64)
        dists = np.full((nq, top_k), np.inf, np.float32)
        counts = np.zeros(nq, np.uint32)
        N.check(N.lib().leann_backend_search_filtered_batch(self._h, _p(Q, f32p), nq, top_k, complexity, _p(allow, u8p),
                                                            stride, _p(keys, u64p), _p(dists, f32p), _p(counts, u32p)))
        return keys, dists, counts

    def search_filtered_exact_batch(self, queries, top_k, allow):
        """exact answer for a selective filter: the allowed rows are compacted and scanned (no graph).  allow as in
        search_filtered_batch."""
        Q = np.ascontiguousarray(queries, np.float32)
        if Q.ndim != 2 or Q.shape[1] != self.dims():
            raise LeannError(1, f"queries must be [nq x {self.dims()}]")
        allow = np.ascontiguousarray(allow, np.uint8)
        stride = 0 if allow.ndim == 1 else allow.shape[1]
        if allow.shape[-1] < (self.len() + 7) // 8 or (allow.ndim == 2 and allow.shape[0] != Q.shape[0]):
            raise LeannError(1, "allow-bitmap shape does not match the index / the batch")
        nq = Q.shape[0]
        keys = np.full((nq, top_k), np.iinfo(np.uint64).max, np.uint64)
        dists = np.full((nq, top_k), np.inf, np.float32)
        counts = np.zeros(nq, np.uint32)
        N.check(N.lib().leann_backend_search_filtered_exact_batch(self._h, _p(Q, f32p), nq, top_k, _p(allow, u8p), stride,
                                                                  _p(keys, u64p), _p(dists, f32p), _p(counts, u32p)))
        return keys, dists, counts

    def search_filtered_exact_batch_device(self, d_queries, nq, top_k, d_allow, allow_stride, d_keys, d_dists, d_counts,
                                           stream=None):
        N.check(N.lib().leann_backend_search_filtered_exact_batch_device(self._h, d_queries, nq, top_k, d_allow, allow_stride,
                                                                         d_keys, d_dists, d_counts, stream))

    def register_filter(self, allow):
        """upload + compact an allow-bitmap once; returns a Filter for search_filter_batch (close() it when done)"""
        allow = np.ascontiguousarray(allow, np.uint8)
        if allow.ndim != 1 or allow.shape[0] < (self.len() + 7) // 8:
            raise LeannError(1, "allow-bitmap shape does not match the index")
        h = C.c_void_p()
        N.check(N.lib().leann_backend_filter_create(self._h, _p(allow, u8p), C.byref(h)))
        return Filter(h)

    def register_meta_filter(self, meta, flt):
        """register_filter with the bitmap evaluated on the device from a metadata.MetaColumns store; `flt`: a filter tree or its text"""
        from .metadata import encode_tree
        nodes, k, keep = encode_tree(flt)
        h = C.c_void_p()
        N.check(N.lib().leann_backend_filter_create_meta(self._h, meta._h, nodes, k, C.byref(h)))
        del keep
        return Filter(h)

    def search_meta_batch(self, meta, queries, filters, top_k, complexity, mode="walk"):
        """nq queries, query i under filters[i] (trees or their text) evaluated on the device from a metadata.MetaColumns store;
        mode: "walk" | "exact".  Returns keys, dists, counts and the rows each filter allows."""
        from .metadata import encode_trees
        Q = np.ascontiguousarray(queries, np.float32)
        if Q.ndim != 2 or Q.shape[1] != self.dims():
            raise LeannError(1, f"queries must be [nq x {self.dims()}]")
        nq = Q.shape[0]
        if len(filters) != nq:
            raise LeannError(1, f"{len(filters)} filters for {nq} queries")
        nodes, off, _, keep = encode_trees(filters)
        keys = np.full((nq, top_k), np.iinfo(np.uint64).max, np.uint64)
        dists = np.full((nq, top_k), np.inf, np.float32)
        counts = np.zeros(nq, np.uint32)
        allowed = np.zeros(nq, np.uint32)
        N.check(N.lib().leann_backend_search_meta_batch(self._h, meta._h, _p(Q, f32p), nq, top_k, complexity, nodes, off,
                                                        {"walk": 0, "exact": 1}[mode], _p(keys, u64p), _p(dists, f32p), _p(counts, u32p),
                                                        None, _p(allowed, u32p)))
        del keep
        return keys, dists, counts, allowed

    def search_meta_batch_device(self, meta, d_queries, nq, filters, top_k, complexity, d_keys, d_dists, d_counts, d_stats=None,
                                 d_n_allowed=None, mode="walk", stream=None):
        """the same with device pointers (ints); synchronises `stream` before it returns.  mode may also be given as its number."""
        from .metadata import encode_trees
        if len(filters) != nq:
            raise LeannError(1, f"{len(filters)} filters for {nq} queries")
        nodes, off, _, keep = encode_trees(filters)
        N.check(N.lib().leann_backend_search_meta_batch_device(self._h, meta._h, d_queries, nq, top_k, complexity, nodes, off,
                                                               {"walk": 0, "exact": 1}.get(mode, mode), d_keys, d_dists, d_counts,
                                                               d_stats, d_n_allowed, stream))
        del keep

    def search_filter_batch(self, queries, top_k, complexity, flt, mode="auto"):
        """nq queries under a registered filter; mode: "walk" | "exact" | "auto" (the library chooses by the filter's selectivity)"""
        Q = np.ascontiguousarray(queries, np.float32)
        if Q.ndim != 2 or Q.shape[1] != self.dims():
            raise LeannError(1, f"queries must be [nq x {self.dims()}]")
        nq = Q.shape[0]
        keys = np.full((nq, top_k), np.iinfo(np.uint64).max, np.uint64)
        dists = np.full((nq, top_k), np.inf, np.float32)
        counts = np.zeros(nq, np.uint32)
        N.check(N.lib().leann_backend_search_filter_batch(self._h, _p(Q, f32p), nq, top_k, complexity, flt._h,
                                                          {"walk": 0, "exact": 1, "auto": 2}[mode], _p(keys, u64p), _p(dists, f32p),
                                                          _p(counts, u32p)))
        return keys, dists, counts

    def search_batch_device(self, d_queries, nq, top_k, complexity, d_keys, d_dists, d_counts,
                            d_stats=None, stream=None):
        N.check(N.lib().leann_backend_search_batch_device(self._h, d_queries, nq, top_k, complexity,
                                                          d_keys, d_dists, d_counts, d_stats, stream))

    def search_filtered_batch_device(self, d_queries, nq, top_k, complexity, d_allow, allow_stride, d_keys, d_dists,
                                     d_counts, d_stats=None, stream=None):
        N.check(N.lib().leann_backend_search_filtered_batch_device(self._h, d_queries, nq, top_k, complexity, d_allow,
                                                                   allow_stride, d_keys, d_dists, d_counts, d_stats, stream))

    def search_refined_batch(self, queries, top_k, fetch_k, complexity, rows, allow=None):
        """the walk at top_k = fetch_k, then its candidates scored again on the exact rows of an ExactRows: the best top_k by the
        f32 distance.  allow: None, or as in search_filtered_batch.  Returns keys, dists, counts."""
        Q = np.ascontiguousarray(queries, np.float32)
        if Q.ndim != 2 or Q.shape[1] != self.dims():
            raise LeannError(1, f"queries must be [nq x {self.dims()}]")
        nq, stride = Q.shape[0], 0
        if allow is not None:
            allow = np.ascontiguousarray(allow, np.uint8)
            stride = 0 if allow.ndim == 1 else allow.shape[1]
            if allow.shape[-1] < (self.len() + 7) // 8 or (allow.ndim == 2 and allow.shape[0] != nq):
                raise LeannError(1, "allow-bitmap shape does not match the index / the batch")
        keys = np.full((nq, max(top_k, 1)), np.iinfo(np.uint64).max, np.uint64)
        dists = np.full((nq, max(top_k, 1)), np.inf, np.float32)
        counts = np.zeros(nq, np.uint32)
        N.check(N.lib().leann_backend_search_refined_batch(self._h, rows._h, _p(Q, f32p), nq, top_k, fetch_k, complexity,
                                                           _p(allow, u8p), stride, _p(keys, u64p), _p(dists, f32p), _p(counts, u32p),
                                                           None))
        return keys, dists, counts

    def search_refined_batch_device(self, rows, d_queries, nq, top_k, fetch_k, complexity, d_keys, d_dists, d_counts, d_allow=None,
                                    allow_stride=0, d_stats=None, stream=None):
        """the same with device pointers (ints); synchronises `stream` before it returns"""
        N.check(N.lib().leann_backend_search_refined_batch_device(self._h, rows._h, d_queries, nq, top_k, fetch_k, complexity, d_allow,
                                                                  allow_stride, d_keys, d_dists, d_counts, d_stats, stream))

    def set_coalescing(self, wait_us=200, max_batch=4096):
        """gather concurrent single-query search() callers into one batched launch ((0, 0) disables)"""
        N.check(N.lib().leann_backend_set_coalescing(self._h, wait_us, max_batch))

    def coalescing_stats(self):
        a, b = C.c_uint64(0), C.c_uint64(0)
        N.check(N.lib().leann_backend_coalescing_stats(self._h, C.byref(a), C.byref(b)))
        return {"launches": a.value, "queries": b.value}

    def set_row_screen(self, enable=True):
        """split-plane row screen of large unfiltered batches on / off (results are bit-identical either way)"""
        N.check(N.lib().leann_backend_set_row_screen(self._h, 1 if enable else 0))

    def row_screen_stats(self):
        out = (C.c_uint64 * 2)()
        N.check(N.lib().leann_backend_row_screen_stats(self._h, out))
        return {"ruled_out": int(out[0]), "read_in_full": int(out[1])}

    def len(self):
        return int(N.lib().leann_backend_len(self._h))

    __len__ = len

    def is_empty(self):
        return self.len() == 0

    def dims(self):
        return int(N.lib().leann_backend_dims(self._h))

    # -- removals (additive) -------------------------------------------------------
    def remove(self, keys):
        """mark keys (global positions) as removed; every search excludes them from now on.  Returns how many were newly removed."""
        k = np.ascontiguousarray(keys, np.uint64).reshape(-1)
        n = C.c_size_t(0)
        N.check(N.lib().leann_backend_remove(self._h, _p(k, u64p), k.shape[0], C.byref(n)))
        return int(n.value)

    def consolidate(self):
        """repair the graph on the device so that no live list names a removed position"""
        N.check(N.lib().leann_backend_consolidate(self._h))

    def live_len(self):
        return int(N.lib().leann_backend_live_len(self._h))

    def removed_bitmap(self):
        """(bitmap [ceil(len/8)] uint8, bit set = removed; number of removed positions live lists still name)"""
        bm = np.zeros(max((self.len() + 7) // 8, 1), np.uint8)
        pend = C.c_size_t(0)
        N.check(N.lib().leann_backend_removed_bitmap(self._h, _p(bm, u8p), C.byref(pend)))
        return bm[: (self.len() + 7) // 8], int(pend.value)

    def compact(self, key_offset=None):
        """(a new searcher of the same class over the live positions only, renumbered 0 .. live-1 in their old order; new_to_old
        [live] uint64: the OLD global key of every new position).  Needs a consolidated handle; this one is left as it is.
        key_offset: the new searcher's (None: this one's)."""
        if key_offset is None:
            key_offset = np.iinfo(np.uint64).max  # LEANN_KEY_OFFSET_KEEP
        m = np.zeros(max(self.live_len(), 1), np.uint64)
        h = C.c_void_p()
        N.check(N.lib().leann_backend_compact(self._h, int(key_offset), C.byref(h), _p(m, u64p)))
        s = type(self)(h, self.backend_type)
        return s, m[: s.len()]

    def append(self, vectors):
        """a new searcher of the same class over this one's positions plus the rows of `vectors` [n x dims] (host), whose keys
        continue the sequence; the graph is this one's, continued by the builder.  This searcher is left as it is."""
        X = np.ascontiguousarray(vectors, np.float32)
        if X.ndim != 2 or X.shape[1] != self.dims():
            raise LeannError(1, f"vectors must be [n x {self.dims()}]")
        h = C.c_void_p()
        N.check(N.lib().leann_backend_append(self._h, _p(X, f32p) if X.shape[0] else None, X.shape[0], C.byref(h)))
        return type(self)(h, self.backend_type)

    def append_device(self, d_vectors_ptr, n, ld):
        """append() for n rows already on this searcher's device: [n x ld] f32, ld >= dims, ld % 4 == 0"""
        h = C.c_void_p()
        N.check(N.lib().leann_backend_append_device(self._h, d_vectors_ptr, n, ld, C.byref(h)))
        return type(self)(h, self.backend_type)

    # -- extras -------------------------------------------------------------------------------
    def stats(self, reset=False):
        s = N.SearchStats()
        N.check(N.lib().leann_backend_stats(self._h, C.byref(s), 1 if reset else 0))
        return {k: int(getattr(s, k)) for k, _ in N.SearchStats._fields_}

    def graph_info(self):
        info = np.zeros(8, np.uint64)
        N.check(N.lib().leann_backend_graph_info(self._h, _p(info, u64p)))
        names = ("n", "dims", "ld", "M", "M0", "max_level", "entry", "n_upper_lists")
        return {k: int(v) for k, v in zip(names, info)}

    def graph_export(self, with_vectors=False):
        gi = self.graph_info()
        n = gi["n"]
        levels = np.zeros(n, np.uint8)
        upper_off = np.zeros(n, np.uint32)
        adj0 = np.zeros((n, gi["M0"]), np.uint32)
        adjU = np.zeros((max(gi["n_upper_lists"], 1), gi["M"]), np.uint32)
        X = np.zeros((n, gi["dims"]), np.float32) if with_vectors else None
        N.check(N.lib().leann_backend_graph_export(self._h, _p(levels, u8p), _p(upper_off, u32p),
                                                   _p(adj0, u32p), _p(adjU, u32p), _p(X, f32p)))
        return dict(gi, levels=levels, upper_off=upper_off, adj0=adj0, adjU=adjU[: gi["n_upper_lists"]],
                    vectors=X)

    def n_shards(self):
        """0 for a plain handle; G for a composite (sharded) one"""
        return int(N.lib().leann_backend_shard_count(self._h))

    def shard(self, g):
        """the sub-index of shard g as an ordinary searcher (borrowed: valid while this handle lives; never closed by itself)"""
        h = C.c_void_p()
        N.check(N.lib().leann_backend_shard(self._h, g, C.byref(h)))
        s = BackendSearcher(h, self.backend_type)
        s._borrowed = True
        return s

    def row_type(self):
        return RowType(N.lib().leann_backend_row_type(self._h))

    def to_rows(self, row_type):
        """a new searcher with the same graph and this one's rows in another type (f32 -> bf16, f32 -> int8)"""
        h = C.c_void_p()
        N.check(N.lib().leann_backend_to_rows(self._h, int(row_type), C.byref(h)))
        return BackendSearcher(h, self.backend_type)

    def export_rows_bf16(self):
        """the rows of a bf16 index as stored: [n x dims] uint16"""
        out = np.zeros((self.len(), self.dims()), np.uint16)
        N.check(N.lib().leann_backend_rows_export_bf16(self._h, out.ctypes.data_as(C.POINTER(C.c_uint16))))
        return out

    def rows_export_i8(self):
        """the rows of an int8 index as stored: (exps int8 [dims], codes int8 [n x dims])"""
        exps, codes = np.zeros(self.dims(), np.int8), np.zeros((self.len(), self.dims()), np.int8)
        i8p = C.POINTER(C.c_int8)
        N.check(N.lib().leann_backend_rows_export_i8(self._h, exps.ctypes.data_as(i8p), codes.ctypes.data_as(i8p)))
        return exps, codes

    def device_rows_ptr(self):
        return N.lib().leann_backend_device_rows(self._h)

    def save(self, index_path):
        N.check(N.lib().leann_backend_save(self._h, os.fsencode(str(index_path))))

    def close(self):
        if self._h:
            if not getattr(self, "_borrowed", False):
                N.lib().leann_backend_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HnswSearcher(BackendSearcher):
    """src/backend/hnsw.rs:12-14"""

    @classmethod
    def load(cls, index_path, dimensions, device=0):
        return BackendSearcher.load.__func__(cls, BackendType.Hnsw, index_path, dimensions, device)


class DiskAnnSearcher(BackendSearcher):
    """src/backend/diskann.rs:15-17"""

    @classmethod
    def load(cls, index_path, dimensions, device=0):
        return BackendSearcher.load.__func__(cls, BackendType.DiskAnn, index_path, dimensions, device)


class BackendBuilder:
    """struct BackendBuilder — src/backend/traits.rs:6-8, impl src/backend/mod.rs:48-101"""

    def __init__(self, backend_type):
        self.backend_type = BackendType(backend_type)

    def build(self, embeddings, ids, index_path, dimensions, graph_degree, complexity, row_type=RowType.F32):
        """mod.rs:55-79 -> hnsw.rs:96-139 / diskann.rs:70-105.  `ids` is unused, as in the reference."""
        X = np.ascontiguousarray(embeddings, np.float32)
        if X.ndim != 2 or X.shape[1] != dimensions:
            raise LeannError(1, f"embeddings must be [n x {dimensions}]")
        if int(row_type) != RowType.F32:
            N.check(N.lib().leann_backend_build_rows(int(self.backend_type), _p(X, f32p), X.shape[0], dimensions,
                                                     graph_degree, complexity, int(row_type), os.fsencode(str(index_path))))
            return
        N.check(N.lib().leann_backend_build(int(self.backend_type), _p(X, f32p), X.shape[0], dimensions,
                                            graph_degree, complexity, os.fsencode(str(index_path))))

    def add_to_index(self, embeddings, index_path, dimensions, start_id):
        """mod.rs:82-100 -> hnsw.rs:142-191; DiskANN refuses (mod.rs:93-98)."""
        X = np.ascontiguousarray(embeddings, np.float32)
        N.check(N.lib().leann_backend_add(int(self.backend_type), _p(X, f32p), X.shape[0], dimensions,
                                          start_id, os.fsencode(str(index_path))))

    def remove_from_index(self, keys, index_path, dimensions):
        """the file twin of BackendSearcher.remove + consolidate: open -> remove -> consolidate -> save"""
        k = np.ascontiguousarray(keys, np.uint64).reshape(-1)
        N.check(N.lib().leann_backend_remove_from_index(int(self.backend_type), _p(k, u64p), k.shape[0], dimensions,
                                                        os.fsencode(str(index_path))))

    def compact_index(self, index_path, dimensions):
        """the file twin of BackendSearcher.compact: open -> consolidate if need be -> compact -> save.  Returns new_to_old [live]
        uint64 (the identity, and an untouched file, when nothing was removed)."""
        stem = os.fsencode(str(index_path))
        live = C.c_size_t(0)
        m = np.zeros(1, np.uint64)
        # a map without room changes nothing and reports the size needed (a file that does not open raises here)
        rc = N.lib().leann_backend_compact_index(int(self.backend_type), dimensions, stem, _p(m, u64p), 0, C.byref(live))
        if rc != 0 and live.value == 0:
            N.check(rc)
        m = np.zeros(max(live.value, 1), np.uint64)
        N.check(N.lib().leann_backend_compact_index(int(self.backend_type), dimensions, stem, _p(m, u64p), m.shape[0], C.byref(live)))
        return m[: live.value]


class Filter:
    """a metadata filter registered on the device (leann_backend_filter_create)"""

    def __init__(self, handle):
        self._h = handle

    def count(self):
        return int(N.lib().leann_backend_filter_count(self._h))

    def device_bitmap(self):
        """(device pointer, positions) of the registered bitmap — valid AND match AND live — borrowed until close(): an allow-bitmap
        for Bm25Index.search_batch_device / hybrid_rerank_device.  The filter of a composite handle has none (LeannError 5)."""
        p, n = C.c_void_p(), C.c_size_t(0)
        N.check(N.lib().leann_backend_filter_bitmap_device(self._h, C.byref(p), C.byref(n)))
        return p.value, int(n.value)

    def close(self):
        if self._h:
            N.lib().leann_backend_filter_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ExactRows:
    """exact f32 rows to refine search results on (leann_exact_rows, include/leann_backend.h "refining results on exact rows"):
    placement "hbm" keeps them in device memory, "host" in pinned host memory the rerank kernel reads in place"""
    PLACEMENTS = {"hbm": 0, "host": 1}

    def __init__(self, handle, keep=None):
        self._h = handle
        self._keep = keep  # from_device: whatever owns the borrowed rows

    @classmethod
    def _placement(cls, placement):
        if isinstance(placement, str) and placement not in cls.PLACEMENTS:
            raise LeannError(1, f"placement = {placement!r} is neither 'hbm' nor 'host'")
        return cls.PLACEMENTS.get(placement, placement)  # (an unknown number goes to the library, which refuses it)

    @classmethod
    def from_host(cls, X, device=0, key_offset=0, placement="hbm"):
        X = np.ascontiguousarray(X, np.float32)
        if X.ndim != 2:
            raise LeannError(1, "ExactRows.from_host: rows must be [n x dims]")
        h = C.c_void_p()
        N.check(N.lib().leann_exact_rows_from_host(_p(X, f32p), X.shape[0], X.shape[1], device, key_offset, cls._placement(placement),
                                                   C.byref(h)))
        return cls(h)

    @classmethod
    def from_device(cls, d_rows_ptr, n, dims, ld, device=0, key_offset=0, keep=None):
        """borrowed rows [n x ld] on `device` (e.g. BackendSearcher.device_rows_ptr() of an f32 index): they must outlive this object"""
        h = C.c_void_p()
        N.check(N.lib().leann_exact_rows_from_device(d_rows_ptr, n, dims, ld, device, key_offset, C.byref(h)))
        return cls(h, keep)

    @classmethod
    def open(cls, path, dims, device=0, key_offset=0, placement="hbm"):
        """a "<stem>.embeddings" file: raw f32 [n x dims], as `leann build --recompute` writes it beside the index"""
        h = C.c_void_p()
        N.check(N.lib().leann_exact_rows_open(os.fsencode(str(path)), dims, device, key_offset, cls._placement(placement), C.byref(h)))
        return cls(h)

    def len(self):
        return int(N.lib().leann_exact_rows_len(self._h))

    __len__ = len

    def placement(self):
        return {0: "hbm", 1: "host"}[N.lib().leann_exact_rows_placement(self._h)]

    def close(self):
        if self._h:
            N.lib().leann_exact_rows_close(self._h)
            self._h = None
            self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def rerank_batch_device(rows, d_queries, nq, d_keys, d_counts, fetch_k, top_k, d_out_keys, d_out_dists, d_out_counts, d_skipped=None,
                        stream=None):
    """leann_rerank_batch_device: the candidate lists d_keys [nq x fetch_k] scored on the exact rows, best top_k out; device pointers
    (ints).  Only enqueues on `stream`."""
    N.check(N.lib().leann_rerank_batch_device(rows._h, d_queries, nq, d_keys, d_counts, fetch_k, top_k, d_out_keys, d_out_dists,
                                              d_out_counts, d_skipped, stream))


class ShardedIndex:
    """leann_sharded (include/leann_backend.h "sharded indexes", csrc/shard.hip): the corpus partitioned into contiguous position
    ranges, one sub-index per shard; a search = per-shard traversal + gather of the per-shard lists + merge kernel.  One process
    over several devices (open / build_device / from_searchers) or one process per GPU over RCCL (attach)."""

    def __init__(self, handle, keep=()):
        self._h = handle
        self._keep = keep  # objects whose device memory the shards borrow

    @classmethod
    def open(cls, backend_type, index_path, dimensions, device_spec):
        h = C.c_void_p()
        N.check(N.lib().leann_sharded_open(os.fsencode(str(index_path)), int(backend_type), dimensions, str(device_spec).encode(), C.byref(h)))
        return cls(h)

    @classmethod
    def build_device(cls, backend_type, d_ptrs, rows, dims, ld, graph_degree, complexity, devices, keep=()):
        G = len(d_ptrs)
        ptrs = (C.c_void_p * G)(*[C.c_void_p(p) for p in d_ptrs])
        rws = (C.c_size_t * G)(*rows)
        devs = (C.c_int * G)(*devices)
        h = C.c_void_p()
        N.check(N.lib().leann_sharded_build_device(int(backend_type), ptrs, rws, G, dims, ld, graph_degree, complexity, devs, C.byref(h)))
        return cls(h, keep)

    @classmethod
    def from_searchers(cls, searchers, take_ownership=False):
        G = len(searchers)
        hs = (C.c_void_p * G)(*[s._h for s in searchers])
        h = C.c_void_p()
        N.check(N.lib().leann_sharded_from_handles(hs, G, 1 if take_ownership else 0, C.byref(h)))
        if take_ownership:
            for s in searchers:
                s._h = None
        return cls(h, tuple(searchers))

    @staticmethod
    def rccl_unique_id():
        """128 opaque bytes made by rank 0; the host distributes them to the other ranks by its own means"""
        buf = C.create_string_buffer(128)
        N.check(N.lib().leann_rccl_get_unique_id(buf))
        return buf.raw

    @classmethod
    def attach(cls, searcher, unique_id, world, rank, total_rows=0):
        """join this rank's shard to the RCCL group (collective: every rank calls it)"""
        h = C.c_void_p()
        N.check(N.lib().leann_sharded_attach(searcher._h, C.c_char_p(bytes(unique_id)), world, rank, total_rows, C.byref(h)))
        return cls(h, (searcher,))

    def search_batch_device(self, d_queries, nq, top_k, complexity, d_keys, d_dists, d_counts, d_stats=None, stream=None):
        N.check(N.lib().leann_sharded_search_batch_device(self._h, d_queries, nq, top_k, complexity, d_keys, d_dists, d_counts, d_stats, stream))

    def search_batch_device_async(self, d_queries, nq, top_k, complexity, d_keys, d_dists, d_counts, d_stats=None, stream=None):
        """traversal queued behind `stream`, exchange + merge on the handle's own stream; returns a ticket for wait()"""
        t = C.c_uint64(0)
        N.check(N.lib().leann_sharded_search_batch_device_async(self._h, d_queries, nq, top_k, complexity, d_keys, d_dists, d_counts, d_stats,
                                                                stream, C.byref(t)))
        return t.value

    def wait(self, ticket, stream=None):
        N.check(N.lib().leann_sharded_wait(self._h, ticket, stream))

    def as_backend(self, backend_type=BackendType.Hnsw):
        """the same group as an ordinary BackendSearcher handle (closing it closes the group)"""
        h = C.c_void_p()
        N.check(N.lib().leann_sharded_as_backend(self._h, C.byref(h)))
        keep, self._h = self._keep, None
        s = BackendSearcher(h, backend_type)
        s._keep = keep
        return s

    def len(self):
        return int(N.lib().leann_sharded_len(self._h))

    def n_shards(self):
        return int(N.lib().leann_sharded_shards(self._h))

    def close(self):
        if self._h:
            N.lib().leann_sharded_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
