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


def quantize_query_i8(q, exps):
    """one query [d] and an int8 index's column exponents [d] -> (codes int8 [d] in element order, E): the query codes of the flat
    search (include/leann_backend.h "exhaustive search on int8 rows"), the library's own reference, on the host; E is
    -2**31 and the codes are zero for a query whose scaled elements are not all finite"""
    q = np.ascontiguousarray(q, np.float32).reshape(-1)
    exps = np.ascontiguousarray(exps, np.int8).reshape(-1)
    if q.shape != exps.shape:
        raise LeannError(1, "quantize_query_i8: the query and the exponents differ in length")
    codes, E = np.zeros(q.shape[0], np.int8), C.c_int32(0)
    i8p = C.POINTER(C.c_int8)
    N.check(N.lib().leann_quantize_query_i8(_p(q, f32p), q.shape[0], exps.ctypes.data_as(i8p), codes.ctypes.data_as(i8p), C.byref(E)))
    return codes, E.value


def split_query_bf16(q):
    """one query [d] -> (hi, lo) uint16 [d] in element order: the two bf16 pieces hi = r(q), lo = r(q - w(hi)) of the flat search on
    bf16 rows (include/leann_backend.h "exhaustive search on bf16 rows"), the library's own reference, on the host"""
    q = np.ascontiguousarray(q, np.float32).reshape(-1)
    hi, lo = np.zeros(q.shape[0], np.uint16), np.zeros(q.shape[0], np.uint16)
    u16p = C.POINTER(C.c_uint16)
    N.check(N.lib().leann_split_query_bf16(_p(q, f32p), q.shape[0], hi.ctypes.data_as(u16p), lo.ctypes.data_as(u16p)))
    return hi, lo


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

    def search_exact_lists_batch(self, queries, top_k, lists, q_list=None):
        """exact answer of query i over the positions of lists[q_list[i]] (q_list None: lists[i]); lists: a sequence of uint32 position
        arrays, unsorted and with duplicates if the caller likes.  Returns keys, dists, counts and, per query, how many listed positions
        lay beyond the index."""
        Q = np.ascontiguousarray(queries, np.float32)
        if Q.ndim != 2 or Q.shape[1] != self.dims():
            raise LeannError(1, f"queries must be [nq x {self.dims()}]")
        parts = [np.ascontiguousarray(l, np.uint32).reshape(-1) for l in lists]
        off = np.zeros(len(parts) + 1, np.uint64)
        off[1:] = np.cumsum([p.shape[0] for p in parts], dtype=np.uint64)
        flat = np.concatenate(parts) if parts else np.zeros(0, np.uint32)
        flat = np.ascontiguousarray(flat if flat.size else np.zeros(1, np.uint32), np.uint32)
        ql = None if q_list is None else np.ascontiguousarray(q_list, np.uint32)
        if ql is not None and ql.shape != (Q.shape[0],):
            raise LeannError(1, "q_list must hold one list number per query")
        nq = Q.shape[0]
        keys = np.full((nq, top_k), np.iinfo(np.uint64).max, np.uint64)
        dists = np.full((nq, top_k), np.inf, np.float32)
        counts = np.zeros(nq, np.uint32)
        skipped = np.zeros(nq, np.uint32)
        N.check(N.lib().leann_backend_search_exact_lists_batch(self._h, _p(Q, f32p), nq, top_k, _p(off, u64p), _p(flat, u32p), len(parts),
                                                               None if ql is None else _p(ql, u32p), _p(keys, u64p), _p(dists, f32p),
                                                               _p(counts, u32p), _p(skipped, u32p)))
        return keys, dists, counts, skipped

    def search_exact_lists_batch_device(self, d_queries, nq, top_k, list_off, d_lists, n_lists, q_list, d_keys, d_dists, d_counts,
                                        d_skipped=None, stream=None):
        """list_off (uint64 [n_lists + 1]) and q_list (uint32 [nq] or None) are host arrays, everything else device pointers"""
        off = np.ascontiguousarray(list_off, np.uint64)
        ql = None if q_list is None else np.ascontiguousarray(q_list, np.uint32)
        N.check(N.lib().leann_backend_search_exact_lists_batch_device(self._h, d_queries, nq, top_k, _p(off, u64p), d_lists, n_lists,
                                                                      None if ql is None else _p(ql, u32p), d_keys, d_dists, d_counts,
                                                                      d_skipped, stream))

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

    def search_flat_batch(self, queries, top_k, fetch_k, allow=None):
        """int8 handles: every live and allowed row screened by the int32 dot product of query codes and row codes, the fetch_k best
        scored with the walk's distance, the best top_k returned.  allow: None or ONE bitmap [ceil(len/8)] for the batch."""
        Q = np.ascontiguousarray(queries, np.float32)
        if Q.ndim != 2 or Q.shape[1] != self.dims():
            raise LeannError(1, f"queries must be [nq x {self.dims()}]")
        if allow is not None:
            allow = np.ascontiguousarray(allow, np.uint8)
            if allow.ndim != 1 or allow.shape[0] < (self.len() + 7) // 8:
                raise LeannError(1, "allow-bitmap must be one bitmap of ceil(len / 8) bytes")
        nq = Q.shape[0]
        keys = np.full((nq, max(top_k, 1)), np.iinfo(np.uint64).max, np.uint64)
        dists = np.full((nq, max(top_k, 1)), np.inf, np.float32)
        counts = np.zeros(nq, np.uint32)
        N.check(N.lib().leann_backend_search_flat_batch(self._h, _p(Q, f32p), nq, top_k, fetch_k, _p(allow, u8p), _p(keys, u64p),
                                                        _p(dists, f32p), _p(counts, u32p)))
        return keys, dists, counts

    def search_flat_batch_device(self, d_queries, nq, top_k, fetch_k, d_keys, d_dists, d_counts, d_allow=None, stream=None):
        """the same with device pointers (ints); synchronises `stream` before it returns"""
        N.check(N.lib().leann_backend_search_flat_batch_device(self._h, d_queries, nq, top_k, fetch_k, d_allow, d_keys, d_dists,
                                                               d_counts, stream))

    def search_flat_bf16_batch(self, queries, top_k, fetch_k, allow=None):
        """bf16 handles: every live and allowed row screened on the bf16 matrix cores by its dot product with the query split into two
        bf16 pieces (not rounded), the fetch_k best scored with the walk's distance, the best top_k returned.  allow: None or ONE bitmap
        [ceil(len/8)] for the batch."""
        Q = np.ascontiguousarray(queries, np.float32)
        if Q.ndim != 2 or Q.shape[1] != self.dims():
            raise LeannError(1, f"queries must be [nq x {self.dims()}]")
        if allow is not None:
            allow = np.ascontiguousarray(allow, np.uint8)
            if allow.ndim != 1 or allow.shape[0] < (self.len() + 7) // 8:
                raise LeannError(1, "allow-bitmap must be one bitmap of ceil(len / 8) bytes")
        nq = Q.shape[0]
        keys = np.full((nq, max(top_k, 1)), np.iinfo(np.uint64).max, np.uint64)
        dists = np.full((nq, max(top_k, 1)), np.inf, np.float32)
        counts = np.zeros(nq, np.uint32)
        N.check(N.lib().leann_backend_search_flat_bf16_batch(self._h, _p(Q, f32p), nq, top_k, fetch_k, _p(allow, u8p), _p(keys, u64p),
                                                             _p(dists, f32p), _p(counts, u32p)))
        return keys, dists, counts

    def search_flat_bf16_batch_device(self, d_queries, nq, top_k, fetch_k, d_keys, d_dists, d_counts, d_allow=None, stream=None):
        """the same with device pointers (ints); synchronises `stream` before it returns"""
        N.check(N.lib().leann_backend_search_flat_bf16_batch_device(self._h, d_queries, nq, top_k, fetch_k, d_allow, d_keys, d_dists,
                                                                    d_counts, stream))

    def search_flat_lists_batch(self, queries, top_k, fetch_k, lists, q_list=None):
        """int8 handles: search_flat_batch with query i screened over the positions of lists[q_list[i]] (q_list None: lists[i]) only;
        lists as in search_exact_lists_batch: uint32 position arrays, unsorted and with duplicates if the caller likes.  Returns keys,
        dists, counts and, per query, how many listed positions lay beyond the index."""
        Q = np.ascontiguousarray(queries, np.float32)
        if Q.ndim != 2 or Q.shape[1] != self.dims():
            raise LeannError(1, f"queries must be [nq x {self.dims()}]")
        parts = [np.ascontiguousarray(l, np.uint32).reshape(-1) for l in lists]
        off = np.zeros(len(parts) + 1, np.uint64)
        off[1:] = np.cumsum([p.shape[0] for p in parts], dtype=np.uint64)
        flat = np.concatenate(parts) if parts else np.zeros(0, np.uint32)
        flat = np.ascontiguousarray(flat if flat.size else np.zeros(1, np.uint32), np.uint32)
        ql = None if q_list is None else np.ascontiguousarray(q_list, np.uint32)
        if ql is not None and ql.shape != (Q.shape[0],):
            raise LeannError(1, "q_list must hold one list number per query")
        nq = Q.shape[0]
        keys = np.full((nq, max(top_k, 1)), np.iinfo(np.uint64).max, np.uint64)
        dists = np.full((nq, max(top_k, 1)), np.inf, np.float32)
        counts = np.zeros(nq, np.uint32)
        skipped = np.zeros(nq, np.uint32)
        N.check(N.lib().leann_backend_search_flat_lists_batch(self._h, _p(Q, f32p), nq, top_k, fetch_k, _p(off, u64p), _p(flat, u32p),
                                                              len(parts), None if ql is None else _p(ql, u32p), _p(keys, u64p),
                                                              _p(dists, f32p), _p(counts, u32p), _p(skipped, u32p)))
        return keys, dists, counts, skipped

    def search_flat_lists_batch_device(self, d_queries, nq, top_k, fetch_k, list_off, d_lists, n_lists, q_list, d_keys, d_dists, d_counts,
                                       d_skipped=None, stream=None):
        """list_off (uint64 [n_lists + 1]) and q_list (uint32 [nq] or None) are host arrays, everything else device pointers;
        synchronises `stream` before it returns"""
        off = np.ascontiguousarray(list_off, np.uint64)
        ql = None if q_list is None else np.ascontiguousarray(q_list, np.uint32)
        N.check(N.lib().leann_backend_search_flat_lists_batch_device(self._h, d_queries, nq, top_k, fetch_k, _p(off, u64p), d_lists, n_lists,
                                                                     None if ql is None else _p(ql, u32p), d_keys, d_dists, d_counts,
                                                                     d_skipped, stream))

    def search_flat_filtered_batch(self, queries, top_k, fetch_k, allow):
        """int8 handles: search_flat_batch with query i under its own bitmap allow[i] ([nq x stride], stride >= ceil(len / 8)); a
        one-dimensional allow is ONE bitmap for the batch, i.e. search_flat_batch.  Per-query metadata filters need no call of their
        own: MetaColumns.eval_batch gives the nq bitmaps for this call, eval_batch_device leaves them on the device for
        search_flat_filtered_batch_device."""
        Q = np.ascontiguousarray(queries, np.float32)
        if Q.ndim != 2 or Q.shape[1] != self.dims():
            raise LeannError(1, f"queries must be [nq x {self.dims()}]")
        allow = np.ascontiguousarray(allow, np.uint8)
        stride = 0 if allow.ndim == 1 else allow.shape[1]
        if allow.shape[-1] < (self.len() + 7) // 8 or (allow.ndim == 2 and allow.shape[0] != Q.shape[0]):
            raise LeannError(1, "allow-bitmap shape does not match the index / the batch")
        nq = Q.shape[0]
        keys = np.full((nq, max(top_k, 1)), np.iinfo(np.uint64).max, np.uint64)
        dists = np.full((nq, max(top_k, 1)), np.inf, np.float32)
        counts = np.zeros(nq, np.uint32)
        N.check(N.lib().leann_backend_search_flat_filtered_batch(self._h, _p(Q, f32p), nq, top_k, fetch_k, _p(allow, u8p), stride,
                                                                 _p(keys, u64p), _p(dists, f32p), _p(counts, u32p)))
        return keys, dists, counts

    def search_flat_filtered_batch_device(self, d_queries, nq, top_k, fetch_k, d_allow, allow_stride, d_keys, d_dists, d_counts,
                                          stream=None):
        """the same with device pointers (ints); allow_stride: bytes from one query's bitmap to the next, 0 for one shared bitmap;
        synchronises `stream` before it returns"""
        N.check(N.lib().leann_backend_search_flat_filtered_batch_device(self._h, d_queries, nq, top_k, fetch_k, d_allow, allow_stride,
                                                                        d_keys, d_dists, d_counts, stream))

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


def pack_sign_bits(x, center=None):
    """f32 rows [n x dims] -> uint8 [n x 16 * ceil(dims / 128)]: bit j of a row is x[j] > center[j] (center None: > 0), little-endian
    within a byte, padding bits zero (include/leann_backend.h "sign-bit rows"): the library's own reference, on the host"""
    x = np.ascontiguousarray(x, np.float32)
    if x.ndim != 2 or x.shape[1] < 1:
        raise LeannError(1, "pack_sign_bits: rows must be [n x dims]")
    center = _center(center, x.shape[1])
    out = np.zeros((x.shape[0], 16 * ((x.shape[1] + 127) // 128)), np.uint8)
    N.check(N.lib().leann_pack_sign_bits(_p(x, f32p), x.shape[0], x.shape[1], _p(center, f32p), _p(out, u8p)))
    return out


def _center(center, dims):
    if center is None:
        return None
    center = np.ascontiguousarray(center, np.float32).reshape(-1)
    if center.shape[0] != dims:
        raise LeannError(1, f"the centre must have {dims} elements")
    return center


class BitRows:
    """sign-bit rows (leann_bit_rows, include/leann_backend.h "sign-bit rows"): one bit per element of f32 rows, searched exhaustively
    on the integer matrix cores; search_refined_batch restores exact distances on an ExactRows"""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def from_host(cls, X, center=None, device=0, key_offset=0):
        X = np.ascontiguousarray(X, np.float32)
        if X.ndim != 2:
            raise LeannError(1, "BitRows.from_host: rows must be [n x dims]")
        h = C.c_void_p()
        N.check(N.lib().leann_bit_rows_from_host(_p(X, f32p), X.shape[0], X.shape[1], _p(_center(center, X.shape[1]), f32p), device,
                                                 key_offset, C.byref(h)))
        return cls(h)

    @classmethod
    def from_device(cls, d_rows_ptr, n, dims, ld, d_center_ptr=None, device=0, key_offset=0):
        """f32 rows [n x ld] (and an optional centre [dims]) on `device`, device pointers (ints): only read, they need not outlive this object"""
        h = C.c_void_p()
        N.check(N.lib().leann_bit_rows_from_device(d_rows_ptr, n, dims, ld, d_center_ptr, device, key_offset, C.byref(h)))
        return cls(h)

    @classmethod
    def from_searcher(cls, searcher, d_center_ptr=None, device=0, key_offset=0):
        """the bits of an f32 index's rows; a handle without f32 rows (bf16, int8, recompute-on, composite) is refused"""
        ptr = searcher.device_rows_ptr()
        if not ptr:
            raise LeannError(1, "BitRows.from_searcher: the index has no f32 rows on one device (leann_backend_device_rows is NULL)")
        return cls.from_device(ptr, searcher.len(), searcher.dims(), searcher.graph_info()["ld"], d_center_ptr, device, key_offset)

    def len(self):
        return int(N.lib().leann_bit_rows_len(self._h))

    __len__ = len

    def dims(self):
        return int(N.lib().leann_bit_rows_dims(self._h))

    def pitch(self):
        return int(N.lib().leann_bit_rows_pitch(self._h))

    def export(self):
        """the rows as uint8 [n x pitch], exactly pack_sign_bits's layout"""
        out = np.zeros((self.len(), self.pitch()), np.uint8)
        N.check(N.lib().leann_bit_rows_export(self._h, _p(out, u8p)))
        return out

    def _host_args(self, queries, allow):
        Q = np.ascontiguousarray(queries, np.float32)
        if Q.ndim != 2 or Q.shape[1] != self.dims():
            raise LeannError(1, f"queries must be [nq x {self.dims()}]")
        if allow is not None:
            allow = np.ascontiguousarray(allow, np.uint8)
            if allow.ndim != 1 or allow.shape[0] < (self.len() + 7) // 8:
                raise LeannError(1, "allow-bitmap must be one bitmap of ceil(len / 8) bytes")
        return Q, allow

    def search_batch(self, queries, fetch_k, allow=None):
        """the fetch_k allowed rows with the largest int32 score per query, ties to the lower position: (keys, scores, counts); the
        tail is UINT64_MAX / -inf.  allow: None or ONE bitmap [ceil(len/8)] for the batch."""
        Q, allow = self._host_args(queries, allow)
        nq = Q.shape[0]
        keys = np.full((nq, max(fetch_k, 1)), np.iinfo(np.uint64).max, np.uint64)
        scores = np.full((nq, max(fetch_k, 1)), -np.inf, np.float32)
        counts = np.zeros(nq, np.uint32)
        N.check(N.lib().leann_bit_rows_search_batch(self._h, _p(Q, f32p), nq, fetch_k, _p(allow, u8p), _p(keys, u64p), _p(scores, f32p),
                                                    _p(counts, u32p)))
        return keys, scores, counts

    def search_batch_device(self, d_queries, nq, fetch_k, d_keys, d_scores, d_counts, d_allow=None, stream=None):
        """the same with device pointers (ints); synchronises `stream` before it returns"""
        N.check(N.lib().leann_bit_rows_search_batch_device(self._h, d_queries, nq, fetch_k, d_allow, d_keys, d_scores, d_counts, stream))

    def search_refined_batch(self, exact_rows, queries, top_k, fetch_k, allow=None):
        """search_batch's candidates scored again on the exact rows of an ExactRows: the best top_k by the f32 distance"""
        Q, allow = self._host_args(queries, allow)
        nq = Q.shape[0]
        keys = np.full((nq, max(top_k, 1)), np.iinfo(np.uint64).max, np.uint64)
        dists = np.full((nq, max(top_k, 1)), np.inf, np.float32)
        counts = np.zeros(nq, np.uint32)
        N.check(N.lib().leann_bit_rows_search_refined_batch(self._h, exact_rows._h if exact_rows is not None else None, _p(Q, f32p), nq,
                                                            top_k, fetch_k, _p(allow, u8p), _p(keys, u64p), _p(dists, f32p),
                                                            _p(counts, u32p)))
        return keys, dists, counts

    def search_refined_batch_device(self, exact_rows, d_queries, nq, top_k, fetch_k, d_keys, d_dists, d_counts, d_allow=None, stream=None):
        """the same with device pointers (ints); synchronises `stream` before it returns"""
        N.check(N.lib().leann_bit_rows_search_refined_batch_device(self._h, exact_rows._h if exact_rows is not None else None, d_queries,
                                                                   nq, top_k, fetch_k, d_allow, d_keys, d_dists, d_counts, stream))

    def close(self):
        if self._h:
            N.lib().leann_bit_rows_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _mx4_ktiles(dims):
    return (dims + 255) // 256


def pack_mx4(x):
    """f32 rows [n x dims] -> (codes uint8 [n x 128 KT], scales uint8 [n x 8 KT]), KT = ceil(dims / 256): E2M1 nibbles, low nibble first,
    and one E8M0 scale byte per 32 elements (include/leann_backend.h "MXFP4 rows"): the library's own reference, on the host"""
    x = np.ascontiguousarray(x, np.float32)
    if x.ndim != 2 or x.shape[1] < 1:
        raise LeannError(1, "pack_mx4: rows must be [n x dims]")
    kt = _mx4_ktiles(x.shape[1])
    codes, scales = np.zeros((x.shape[0], 128 * kt), np.uint8), np.zeros((x.shape[0], 8 * kt), np.uint8)
    N.check(N.lib().leann_pack_mx4(_p(x, f32p), x.shape[0], x.shape[1], _p(codes, u8p), _p(scales, u8p)))
    return codes, scales


def quantize_query_mx8(q):
    """one f32 query -> (codes uint8 [256 KT] in OCP E4M3, scales uint8 [8 KT], finite): the host reference of the MXFP4 search's query
    codes; a query with an element that is not finite has no codes (finite False, codes zero, scales 0xFF)"""
    q = np.ascontiguousarray(q, np.float32).reshape(-1)
    if q.shape[0] < 1:
        raise LeannError(1, "quantize_query_mx8: the query is empty")
    kt = _mx4_ktiles(q.shape[0])
    codes, scales = np.zeros(256 * kt, np.uint8), np.zeros(8 * kt, np.uint8)
    N.check(N.lib().leann_quantize_query_mx8(_p(q, f32p), q.shape[0], _p(codes, u8p), _p(scales, u8p)))
    return codes, scales, bool(scales[0] != 0xFF)


class Mx4Rows:
    """MXFP4 rows (leann_mx4_rows, include/leann_backend.h "MXFP4 rows"): four bits per element and a scale byte per 32 of f32 rows,
    searched exhaustively on the block-scaled matrix cores; search_refined_batch restores exact distances on an ExactRows"""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def from_host(cls, X, device=0, key_offset=0):
        X = np.ascontiguousarray(X, np.float32)
        if X.ndim != 2:
            raise LeannError(1, "Mx4Rows.from_host: rows must be [n x dims]")
        h = C.c_void_p()
        N.check(N.lib().leann_mx4_rows_from_host(_p(X, f32p), X.shape[0], X.shape[1], device, key_offset, C.byref(h)))
        return cls(h)

    @classmethod
    def from_device(cls, d_rows_ptr, n, dims, ld, device=0, key_offset=0):
        """f32 rows [n x ld] on `device`, a device pointer (int): only read, they need not outlive this object"""
        h = C.c_void_p()
        N.check(N.lib().leann_mx4_rows_from_device(d_rows_ptr, n, dims, ld, device, key_offset, C.byref(h)))
        return cls(h)

    @classmethod
    def from_searcher(cls, searcher, device=0, key_offset=0):
        """the codes of an f32 index's rows; a handle without f32 rows (bf16, int8, recompute-on, composite) is refused"""
        ptr = searcher.device_rows_ptr()
        if not ptr:
            raise LeannError(1, "Mx4Rows.from_searcher: the index has no f32 rows on one device (leann_backend_device_rows is NULL)")
        return cls.from_device(ptr, searcher.len(), searcher.dims(), searcher.graph_info()["ld"], device, key_offset)

    def len(self):
        return int(N.lib().leann_mx4_rows_len(self._h))

    __len__ = len

    def dims(self):
        return int(N.lib().leann_mx4_rows_dims(self._h))

    def export(self):
        """(codes uint8 [n x code pitch], scales uint8 [n x scale pitch]), exactly pack_mx4's layout"""
        L = N.lib()
        codes = np.zeros((self.len(), int(L.leann_mx4_rows_code_pitch(self._h))), np.uint8)
        scales = np.zeros((self.len(), int(L.leann_mx4_rows_scale_pitch(self._h))), np.uint8)
        N.check(L.leann_mx4_rows_export(self._h, _p(codes, u8p), _p(scales, u8p)))
        return codes, scales

    _host_args = BitRows._host_args

    def search_batch(self, queries, fetch_k, allow=None):
        """the fetch_k allowed rows with the largest block-scaled score per query, ties to the lower position: (keys, scores,
        counts); the tail is UINT64_MAX / -inf.  allow: None or ONE bitmap [ceil(len/8)] for the batch."""
        Q, allow = self._host_args(queries, allow)
        nq = Q.shape[0]
        keys = np.full((nq, max(fetch_k, 1)), np.iinfo(np.uint64).max, np.uint64)
        scores = np.full((nq, max(fetch_k, 1)), -np.inf, np.float32)
        counts = np.zeros(nq, np.uint32)
        N.check(N.lib().leann_mx4_rows_search_batch(self._h, _p(Q, f32p), nq, fetch_k, _p(allow, u8p), _p(keys, u64p), _p(scores, f32p),
                                                    _p(counts, u32p)))
        return keys, scores, counts

    def search_batch_device(self, d_queries, nq, fetch_k, d_keys, d_scores, d_counts, d_allow=None, stream=None):
        """the same with device pointers (ints); synchronises `stream` before it returns"""
        N.check(N.lib().leann_mx4_rows_search_batch_device(self._h, d_queries, nq, fetch_k, d_allow, d_keys, d_scores, d_counts, stream))

    def search_refined_batch(self, exact_rows, queries, top_k, fetch_k, allow=None):
        """search_batch's candidates scored again on the exact rows of an ExactRows: the best top_k by the f32 distance"""
        Q, allow = self._host_args(queries, allow)
        nq = Q.shape[0]
        keys = np.full((nq, max(top_k, 1)), np.iinfo(np.uint64).max, np.uint64)
        dists = np.full((nq, max(top_k, 1)), np.inf, np.float32)
        counts = np.zeros(nq, np.uint32)
        N.check(N.lib().leann_mx4_rows_search_refined_batch(self._h, exact_rows._h if exact_rows is not None else None, _p(Q, f32p), nq,
                                                            top_k, fetch_k, _p(allow, u8p), _p(keys, u64p), _p(dists, f32p),
                                                            _p(counts, u32p)))
        return keys, dists, counts

    def search_refined_batch_device(self, exact_rows, d_queries, nq, top_k, fetch_k, d_keys, d_dists, d_counts, d_allow=None, stream=None):
        """the same with device pointers (ints); synchronises `stream` before it returns"""
        N.check(N.lib().leann_mx4_rows_search_refined_batch_device(self._h, exact_rows._h if exact_rows is not None else None, d_queries,
                                                                   nq, top_k, fetch_k, d_allow, d_keys, d_dists, d_counts, stream))

    def close(self):
        if self._h:
            N.lib().leann_mx4_rows_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _pq_args(who, x, dsub, codebooks):
    """rows or one query [.. x dims] and codebooks [M x 256 x dsub] as contiguous f32; shapes that do not belong together are refused"""
    x, cb = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(codebooks, np.float32)
    dims = x.shape[-1] if x.ndim else 0
    if dsub not in (4, 8) or dims < 1:
        raise LeannError(1, f"{who}: dsub = {dsub} is neither 4 nor 8" if dims >= 1 else f"{who}: dims = 0")
    if cb.shape != (-(-dims // dsub), 256, dsub):
        raise LeannError(1, f"{who}: codebooks must be [{-(-dims // dsub)} x 256 x {dsub}] for dims = {dims}")
    return x, cb


def pq_train(x, dsub=8, iters=8, device=0):
    """codebooks f32 [M x 256 x dsub] for the sample rows x [n >= 256 x dims] (include/leann_backend.h "PQ rows", step 5): Lloyd
    iterations on the device from the centroids floor(c n / 256), the same bytes on every run; the caller subsamples"""
    x = np.ascontiguousarray(x, np.float32)
    if x.ndim != 2 or x.shape[1] < 1 or dsub not in (4, 8):
        raise LeannError(1, "pq_train: rows must be [n x dims] and dsub 4 or 8")
    cb = np.zeros((-(-x.shape[1] // dsub), 256, dsub), np.float32)
    N.check(N.lib().leann_pq_train(_p(x, f32p), x.shape[0], x.shape[1], dsub, iters, device, _p(cb, f32p)))
    return cb


def pq_encode(x, codebooks, dsub=8):
    """f32 rows [n x dims] -> codes uint8 [n x 16 ceil(M / 16)], the nearest centroid of every sub-space, ties to the lower index: the
    library's own reference, on the host"""
    x, cb = _pq_args("pq_encode", x, dsub, codebooks)
    if x.ndim != 2:
        raise LeannError(1, "pq_encode: rows must be [n x dims]")
    out = np.zeros((x.shape[0], 16 * -(-cb.shape[0] // 16)), np.uint8)
    N.check(N.lib().leann_pq_encode(_p(x, f32p), x.shape[0], x.shape[1], dsub, _p(cb, f32p), _p(out, u8p)))
    return out


def pq_query_lut(q, codebooks, dsub=8):
    """one f32 query -> (tables int16 [M x 256], has_tables): the host reference of the PQ search's query tables; a query with an
    element or a table entry that is not finite has none (tables zero, has_tables False)"""
    q, cb = _pq_args("pq_query_lut", np.asarray(q, np.float32).reshape(-1), dsub, codebooks)
    out = np.zeros((cb.shape[0], 256), np.int16)
    rc = N.lib().leann_pq_query_lut(_p(q, f32p), q.shape[0], dsub, _p(cb, f32p), _p(out, C.POINTER(C.c_int16)))
    if rc == 1 and b"has no tables" in N.lib().leann_last_error():
        return out, False
    N.check(rc)
    return out, True


class PqRows:
    """PQ rows (leann_pq_rows, include/leann_backend.h "PQ rows"): one byte per dsub columns of f32 rows under trained codebooks,
    searched exhaustively by a table gather from LDS; search_refined_batch restores exact distances on an ExactRows"""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def from_host(cls, X, codebooks, dsub=8, device=0, key_offset=0):
        X, cb = _pq_args("PqRows.from_host", X, dsub, codebooks)
        if X.ndim != 2:
            raise LeannError(1, "PqRows.from_host: rows must be [n x dims]")
        h = C.c_void_p()
        N.check(N.lib().leann_pq_rows_from_host(_p(X, f32p), X.shape[0], X.shape[1], _p(cb, f32p), dsub, device, key_offset, C.byref(h)))
        return cls(h)

    @classmethod
    def from_device(cls, d_rows_ptr, n, dims, ld, codebooks, dsub=8, device=0, key_offset=0):
        """f32 rows [n x ld] on `device`, a device pointer (int): only read, they need not outlive this object; codebooks on the host"""
        cb = np.ascontiguousarray(codebooks, np.float32)
        h = C.c_void_p()
        N.check(N.lib().leann_pq_rows_from_device(d_rows_ptr, n, dims, ld, _p(cb, f32p), dsub, device, key_offset, C.byref(h)))
        return cls(h)

    def len(self):
        return int(N.lib().leann_pq_rows_len(self._h))

    __len__ = len

    def dims(self):
        return int(N.lib().leann_pq_rows_dims(self._h))

    def dsub(self):
        return int(N.lib().leann_pq_rows_dsub(self._h))

    def pitch(self):
        return int(N.lib().leann_pq_rows_pitch(self._h))

    def export(self):
        """the codes as uint8 [n x pitch], exactly pq_encode's layout"""
        out = np.zeros((self.len(), self.pitch()), np.uint8)
        N.check(N.lib().leann_pq_rows_export(self._h, _p(out, u8p)))
        return out

    def codebooks(self):
        """the object's copy of the codebooks, f32 [M x 256 x dsub], columns at or behind dims zero"""
        out = np.zeros((-(-self.dims() // self.dsub()), 256, self.dsub()), np.float32)
        N.check(N.lib().leann_pq_rows_codebooks(self._h, _p(out, f32p)))
        return out

    _host_args = BitRows._host_args

    def search_batch(self, queries, fetch_k, allow=None):
        """the fetch_k allowed rows with the largest int32 table sum per query, ties to the lower position: (keys, scores, counts);
        the tail is UINT64_MAX / -inf.  allow: None or ONE bitmap [ceil(len/8)] for the batch."""
        Q, allow = self._host_args(queries, allow)
        nq = Q.shape[0]
        keys = np.full((nq, max(fetch_k, 1)), np.iinfo(np.uint64).max, np.uint64)
        scores = np.full((nq, max(fetch_k, 1)), -np.inf, np.float32)
        counts = np.zeros(nq, np.uint32)
        N.check(N.lib().leann_pq_rows_search_batch(self._h, _p(Q, f32p), nq, fetch_k, _p(allow, u8p), _p(keys, u64p), _p(scores, f32p),
                                                   _p(counts, u32p)))
        return keys, scores, counts

    def search_batch_device(self, d_queries, nq, fetch_k, d_keys, d_scores, d_counts, d_allow=None, stream=None):
        """the same with device pointers (ints); synchronises `stream` before it returns"""
        N.check(N.lib().leann_pq_rows_search_batch_device(self._h, d_queries, nq, fetch_k, d_allow, d_keys, d_scores, d_counts, stream))

    def search_refined_batch(self, exact_rows, queries, top_k, fetch_k, allow=None):
        """search_batch's candidates scored again on the exact rows of an ExactRows: the best top_k by the f32 distance"""
        Q, allow = self._host_args(queries, allow)
        nq = Q.shape[0]
        keys = np.full((nq, max(top_k, 1)), np.iinfo(np.uint64).max, np.uint64)
        dists = np.full((nq, max(top_k, 1)), np.inf, np.float32)
        counts = np.zeros(nq, np.uint32)
        N.check(N.lib().leann_pq_rows_search_refined_batch(self._h, exact_rows._h if exact_rows is not None else None, _p(Q, f32p), nq,
                                                           top_k, fetch_k, _p(allow, u8p), _p(keys, u64p), _p(dists, f32p),
                                                           _p(counts, u32p)))
        return keys, dists, counts

    def search_refined_batch_device(self, exact_rows, d_queries, nq, top_k, fetch_k, d_keys, d_dists, d_counts, d_allow=None, stream=None):
        """the same with device pointers (ints); synchronises `stream` before it returns"""
        N.check(N.lib().leann_pq_rows_search_refined_batch_device(self._h, exact_rows._h if exact_rows is not None else None, d_queries,
                                                                  nq, top_k, fetch_k, d_allow, d_keys, d_dists, d_counts, stream))

    def close(self):
        if self._h:
            N.lib().leann_pq_rows_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


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
