//! MI355X backend for leann-rs — UNCOMPILED source a maintainer would add as `src/backend/gpu.rs` (no Rust toolchain
//! exists in the build image of leann-rs_amd).  Implements the same trait as HnswSearcher /
//! DiskAnnSearcher (src/backend/traits.rs:11-30) over `libleann_hip.so` (include/leann_backend.h).
//!
//! Wiring:
//!   src/backend/mod.rs:23-45   load_searcher:  Hnsw => Box::new(gpu::GpuSearcher::load(index_path, dimensions, 0)?),
//!                                              DiskAnn => Box::new(gpu::GpuSearcher::load(index_path, dimensions, 1)?)
//!   src/backend/mod.rs:55-100  BackendBuilder::{build, add_to_index} => gpu::build / gpu::add_to_index
//!   build.rs                   cargo:rustc-link-search=native=<…>/leann-rs_amd/csrc ; cargo:rustc-link-lib=dylib=leann_hip
//!
//! LEANN_DEVICES: "0" (default) or a list / range ("0-7"): the index is then sharded over those GPUs behind the same handle.
//! LEANN_LOG=info: which file path was taken (own format, cached GPU graph, rebuild from documents.embeddings).
use std::ffi::{c_char, c_int, CStr, CString};
use std::path::Path;

use super::traits::BackendSearcher;

#[repr(C)]
pub struct LeannBackend {
    _p: [u8; 0],
}

#[repr(C)]
pub struct LeannBm25 {
    _p: [u8; 0],
}

// Metadata filters evaluated on the device: a columnar copy of the passages' metadata and the parsed filter tree.
#[repr(C)]
pub struct LeannMeta {
    _p: [u8; 0],
}
#[repr(C)]
pub struct LeannFilter {
    _p: [u8; 0],
}
/// leann_meta_value: type 0 null, 1 bool, 2 number, 3 string (`len` bytes at `str`), 4 list (`len` scalar values at `list`)
#[repr(C)]
pub struct LeannMetaValue {
    pub type_: i32,
    pub boolean: i32,
    pub num: f64,
    pub str_: *const c_char,
    pub len: usize,
    pub list: *const LeannMetaValue,
}
/// leann_meta_node, the MetadataFilter tree in prefix order: kind 0 condition (field, op = FilterOp in declaration order, value),
/// 1 And / 2 Or with `n_children` subtrees behind it
#[repr(C)]
pub struct LeannMetaNode {
    pub kind: i32,
    pub n_children: u32,
    pub field: *const c_char,
    pub op: i32,
    pub value: LeannMetaValue,
}

#[link(name = "leann_hip")]
extern "C" {
    fn leann_last_error() -> *const c_char;
    // BM25 on the device: Bm25Scorer's tables as CSR postings in HBM; a query is its known tokens (term id, idf) in
    // token order.  src/index/searcher.rs:153-167 then becomes one leann_bm25_hybrid_rerank_device call on the backend's lists.
    #[allow(dead_code)]
    pub fn leann_bm25_create(n_docs: usize, n_terms: usize, post_off: *const u64, post_doc: *const u32, post_tf: *const u32,
                             doc_len: *const u32, avg_doc_len: f32, device: c_int, out: *mut *mut LeannBm25) -> c_int;
    #[allow(dead_code)]
    pub fn leann_bm25_search_batch(b: *const LeannBm25, nq: usize, q_off: *const u32, q_term: *const u32, q_idf: *const f32, top_k: usize,
                                   pos: *mut u32, scores: *mut f32, counts: *mut u32, n_positive: *mut u32, min_max: *mut f32) -> c_int;
    #[allow(dead_code)]
    pub fn leann_bm25_hybrid_rerank_device(b: *const LeannBm25, nq: usize, q_off: *const u32, q_term: *const u32, q_idf: *const f32,
                                           d_keys: *const u64, d_dists: *const f32, d_counts: *const u32, fetch_k: usize, alpha: f32,
                                           compat_polarity: c_int, top_k: usize, d_out_keys: *mut u64, d_out_scores: *mut f32,
                                           d_out_counts: *mut u32, stream: *mut std::ffi::c_void) -> c_int;
    #[allow(dead_code)]
    pub fn leann_bm25_close(b: *mut LeannBm25);
    // Metadata filters on the device.  IndexSearcher::load would make the store lazily, beside the passage store: the first filter that
    // names a field costs one pass over the passages extracting that field (tag 0 missing, 1 null, 2 false, 3 true, 4 number, 5 string,
    // 6 array / object; the number as as_f64(); the string's bytes), `valid` = the passages whose metadata could be read.  After that,
    // IndexSearcher::search_with_options (src/index/searcher.rs:123-210) flattens its MetadataFilter into LeannMetaNode and calls
    // leann_backend_filter_create_meta instead of looping over the passages; the LeannFilter goes into the per-filter cache.
    #[allow(dead_code)]
    pub fn leann_meta_create(n: usize, valid: *const u8, device: c_int, out: *mut *mut LeannMeta) -> c_int;
    #[allow(dead_code)]
    pub fn leann_meta_add_column(m: *mut LeannMeta, field: *const c_char, tag: *const u8, num: *const f64, str_blob: *const c_char,
                                 str_off: *const u64) -> c_int;
    #[allow(dead_code)]
    pub fn leann_meta_has_column(m: *const LeannMeta, field: *const c_char) -> c_int;
    #[allow(dead_code)]
    pub fn leann_meta_len(m: *const LeannMeta) -> usize;
    #[allow(dead_code)]
    pub fn leann_meta_close(m: *mut LeannMeta);
    #[allow(dead_code)]
    pub fn leann_meta_eval(m: *const LeannMeta, nodes: *const LeannMetaNode, n_nodes: usize, bitmap: *mut u8, n_allowed: *mut usize) -> c_int;
    #[allow(dead_code)]
    pub fn leann_meta_eval_device(m: *const LeannMeta, nodes: *const LeannMetaNode, n_nodes: usize, d_and: *const u8, d_bitmap: *mut u8,
                                  d_n_allowed: *mut u32, stream: *mut std::ffi::c_void) -> c_int;
    #[allow(dead_code)]
    pub fn leann_backend_filter_create_meta(h: *const LeannBackend, m: *const LeannMeta, nodes: *const LeannMetaNode, n_nodes: usize,
                                            out: *mut *mut LeannFilter) -> c_int;
    #[allow(dead_code)]
    pub fn leann_backend_filter_free(f: *mut LeannFilter);
    fn leann_backend_open(stem: *const c_char, backend: c_int, dims: usize, device_spec: *const c_char,
                          out: *mut *mut LeannBackend) -> c_int;
    fn leann_backend_search(h: *const LeannBackend, query: *const f32, top_k: usize, complexity: usize,
                            keys: *mut u64, dists: *mut f32, n_out: *mut usize) -> c_int;
    #[allow(dead_code)]
    fn leann_backend_set_coalescing(h: *mut LeannBackend, wait_us: u32, max_batch: u32) -> c_int;
    fn leann_backend_len(h: *const LeannBackend) -> usize;
    fn leann_backend_close(h: *mut LeannBackend);
    fn leann_backend_build(backend: c_int, vectors: *const f32, n: usize, dims: usize, graph_degree: usize,
                           complexity: usize, stem: *const c_char) -> c_int;
    fn leann_backend_add(backend: c_int, vectors: *const f32, n: usize, dims: usize, start_id: usize,
                         stem: *const c_char) -> c_int;
    // removals (additive): tombstones + on-device graph repair; keys are global positions, never renumbered
    #[allow(dead_code)]
    fn leann_backend_remove(h: *mut LeannBackend, keys: *const u64, n: usize, n_removed: *mut usize) -> c_int;
    #[allow(dead_code)]
    fn leann_backend_consolidate(h: *mut LeannBackend) -> c_int;
    #[allow(dead_code)]
    fn leann_backend_live_len(h: *const LeannBackend) -> usize;
    #[allow(dead_code)]
    fn leann_backend_removed_bitmap(h: *const LeannBackend, out: *mut u8, n_pending: *mut usize) -> c_int;
    fn leann_backend_remove_from_index(backend: c_int, keys: *const u64, n: usize, dims: usize, stem: *const c_char) -> c_int;
    // compaction (additive): a new handle over the live positions only, renumbered 0 .. live-1 in their old order; new_to_old holds
    // the old global key of every new position
    #[allow(dead_code)]
    fn leann_backend_compact(h: *const LeannBackend, key_offset: u64, out: *mut *mut LeannBackend, new_to_old: *mut u64) -> c_int;
    fn leann_backend_compact_index(backend: c_int, dims: usize, stem: *const c_char, new_to_old: *mut u64, cap: usize,
                                   n_live: *mut usize) -> c_int;
    // row types (additive): 0 = f32 (the default: the calls above), 1 = bf16 rows — half the device memory and index file; a bf16
    // index answers bit for bit like the f32 index over the rounded rows.  leann_backend_open detects the type from the file.
    // 4 = int8 rows — one power-of-two scale per column and 8-bit codes, a quarter of the device memory; the index answers bit for
    // bit like the f32 index over the dequantised rows.  (2 names a recompute-on handle and cannot be asked for; 3 is unassigned.)
    #[allow(dead_code)]
    fn leann_backend_row_type(h: *const LeannBackend) -> c_int;
    #[allow(dead_code)]
    fn leann_round_bf16(input: *const f32, n: usize, out: *mut u16) -> c_int;
    #[allow(dead_code)]
    fn leann_backend_build_rows(backend: c_int, vectors: *const f32, n: usize, dims: usize, graph_degree: usize,
                                complexity: usize, row_type: c_int, stem: *const c_char) -> c_int;
    #[allow(dead_code)]
    fn leann_backend_build_device_rows(backend: c_int, d_vectors: *mut f32, n: usize, dims: usize, ld: usize, graph_degree: usize,
                                       complexity: usize, device: c_int, key_offset: u64, row_type: c_int, may_overwrite: c_int,
                                       out: *mut *mut LeannBackend) -> c_int;
    #[allow(dead_code)]
    fn leann_backend_from_arrays_rows(backend: c_int, vectors: *const f32, n: usize, dims: usize, m: u32, m0: u32, max_level: u32,
                                      entry: u32, levels: *const u8, upper_off: *const u32, adj0: *const u32, adj_u: *const u32,
                                      n_upper_lists: usize, device: c_int, key_offset: u64, row_type: c_int,
                                      out: *mut *mut LeannBackend) -> c_int;
    #[allow(dead_code)]
    fn leann_backend_to_rows(h: *const LeannBackend, row_type: c_int, out: *mut *mut LeannBackend) -> c_int;
    #[allow(dead_code)]
    fn leann_backend_rows_export_bf16(h: *const LeannBackend, out: *mut u16) -> c_int;
    #[allow(dead_code)]
    fn leann_quantize_i8(input: *const f32, n: usize, d: usize, exps: *mut i8, codes: *mut i8) -> c_int;
    #[allow(dead_code)]
    fn leann_backend_rows_export_i8(h: *const LeannBackend, exps: *mut i8, rows: *mut i8) -> c_int;
}

fn last_error() -> anyhow::Error {
    let s = unsafe { CStr::from_ptr(leann_last_error()) }.to_string_lossy().into_owned();
    anyhow::anyhow!(s)
}

pub struct GpuSearcher {
    h: *mut LeannBackend,
}
// leann_backend_search is re-entrant on one handle (per-call workspace + stream inside the library)
unsafe impl Send for GpuSearcher {}
unsafe impl Sync for GpuSearcher {}

impl GpuSearcher {
    /// replaces HnswSearcher::load (hnsw.rs:18-75) / DiskAnnSearcher::load (diskann.rs:21-43); `backend`: 0 = hnsw, 1 = diskann
    pub fn load(index_path: &Path, dimensions: usize, backend: c_int) -> anyhow::Result<Self> {
        let stem = CString::new(index_path.to_string_lossy().as_bytes())?;
        let dev = CString::new(std::env::var("LEANN_DEVICES").unwrap_or_default())?;
        let mut h = std::ptr::null_mut();
        let rc = unsafe { leann_backend_open(stem.as_ptr(), backend, dimensions, dev.as_ptr(), &mut h) };
        if rc != 0 {
            return Err(last_error());
        }
        // a server calls search() from many tokio workers (cli/serve.rs:289-292): the library batches concurrent callers by itself
        // (a lone caller — `leann search` — is answered directly); leann_backend_set_coalescing(h, wait_us, max_batch) only tunes that
        Ok(Self { h })
    }
}

impl BackendSearcher for GpuSearcher {
    fn search(&self, query: &[f32], top_k: usize, complexity: usize) -> anyhow::Result<(Vec<u64>, Vec<f32>)> {
        let (mut keys, mut dists, mut n) = (vec![0u64; top_k], vec![0f32; top_k], 0usize);
        let rc = unsafe {
            leann_backend_search(self.h, query.as_ptr(), top_k, complexity, keys.as_mut_ptr(), dists.as_mut_ptr(), &mut n)
        };
        if rc != 0 {
            return Err(last_error());
        }
        keys.truncate(n);
        dists.truncate(n);
        Ok((keys, dists))
    }

    fn len(&self) -> usize {
        unsafe { leann_backend_len(self.h) }
    }
}

impl Drop for GpuSearcher {
    fn drop(&mut self) {
        unsafe { leann_backend_close(self.h) }
    }
}

fn flatten(embeddings: &[Vec<f32>], dimensions: usize) -> anyhow::Result<Vec<f32>> {
    let mut flat = Vec::with_capacity(embeddings.len() * dimensions);
    for e in embeddings {
        anyhow::ensure!(e.len() == dimensions, "Embedding dimension mismatch: expected {}, got {}", dimensions, e.len());
        flat.extend_from_slice(e);
    }
    Ok(flat)
}

/// BackendBuilder::build (mod.rs:55-79): the graph is built on the GPU and written as "<stem>.index" / ".diskann"
pub fn build(backend: c_int, embeddings: &[Vec<f32>], index_path: &Path, dimensions: usize, graph_degree: usize,
             complexity: usize) -> anyhow::Result<()> {
    let flat = flatten(embeddings, dimensions)?;
    let stem = CString::new(index_path.to_string_lossy().as_bytes())?;
    let rc = unsafe {
        leann_backend_build(backend, flat.as_ptr(), embeddings.len(), dimensions, graph_degree, complexity, stem.as_ptr())
    };
    if rc != 0 {
        return Err(last_error());
    }
    Ok(())
}

/// BackendBuilder::add_to_index (mod.rs:82-100); DiskANN answers with the reference's "does not support incremental updates"
pub fn add_to_index(backend: c_int, embeddings: &[Vec<f32>], index_path: &Path, dimensions: usize, start_id: usize)
                    -> anyhow::Result<()> {
    let flat = flatten(embeddings, dimensions)?;
    let stem = CString::new(index_path.to_string_lossy().as_bytes())?;
    let rc = unsafe { leann_backend_add(backend, flat.as_ptr(), embeddings.len(), dimensions, start_id, stem.as_ptr()) };
    if rc != 0 {
        return Err(last_error());
    }
    Ok(())
}

/// Remove passages (by position) from the index on disk: open -> remove -> consolidate -> save.  Positions keep their numbers.
pub fn remove_from_index(backend: c_int, keys: &[u64], index_path: &Path, dimensions: usize) -> anyhow::Result<()> {
    let stem = CString::new(index_path.to_string_lossy().as_bytes())?;
    let rc = unsafe { leann_backend_remove_from_index(backend, keys.as_ptr(), keys.len(), dimensions, stem.as_ptr()) };
    if rc != 0 {
        return Err(last_error());
    }
    Ok(())
}

/// Compact the index on disk after removals: open -> consolidate if need be -> compact -> save.  Returns new_to_old: entry j is the
/// OLD position of the passage that now sits at position j (ascending; the identity, and an untouched file, when nothing was removed).
///
/// The id map above the backend is positional (searcher.rs:83-92), so the caller applies the map before the next open: the new
/// `<stem>.ids.txt` has line new_to_old[j] of the old one as its line j.  The passage-offset table (`passages.idx.json`) is keyed by
/// passage id, not by position: it stays valid as it is, and the entries of the ids that left `ids.txt` may be dropped from it — the
/// offsets that remain still point into the unchanged `passages.jsonl`, whose removed records are then simply unreferenced (rewriting
/// that file is a separate, optional step).  The passage count in the meta file becomes the map's length.  Write the new `ids.txt`
/// beside the old one and rename it once this call has returned.
pub fn compact_index(backend: c_int, index_path: &Path, dimensions: usize) -> anyhow::Result<Vec<u64>> {
    let stem = CString::new(index_path.to_string_lossy().as_bytes())?;
    // a map without room changes nothing on disk and reports the size needed
    let mut live = 0usize;
    let mut probe = [0u64; 1];
    let rc = unsafe { leann_backend_compact_index(backend, dimensions, stem.as_ptr(), probe.as_mut_ptr(), 0, &mut live) };
    if rc != 0 && live == 0 {
        return Err(last_error());
    }
    let mut map = vec![0u64; live.max(1)];
    let rc = unsafe { leann_backend_compact_index(backend, dimensions, stem.as_ptr(), map.as_mut_ptr(), map.len(), &mut live) };
    if rc != 0 {
        return Err(last_error());
    }
    map.truncate(live);
    Ok(map)
}
