// hybrid.hip — the hybrid leg of IndexSearcher::search_with_options for BATCHES of queries (BASELINE configs[4]: DiskANN + hybrid BM25
// rerank).
//
// Reference, per query (src/index/searcher.rs:146-169, src/index/bm25.rs:135-170):
//     vector_results = backend.search(query, fetch_k = 5 * top_k)              (idx, DISTANCE)          searcher.rs:129-143
//     bm25_scores    = Bm25Scorer::score_query(text)        -> Vec<f32> over ALL N passages              :153
//     bm25_top       = Bm25Scorer::search(text, fetch_k)    -> positives, score desc (stable: index asc) :154, bm25.rs:109-122
//     BM25-only hits are appended with vector score 0.0                                                   :160-165
//     hybrid_rerank: norm_v = (v - min_v) / max(max_v - min_v, 1e-6) over the merged list,
//                    norm_b = (b - min_b) / max(max_b - min_b, 1e-6) with min / max over ALL N scores,
//                    alpha * norm_v + (1 - alpha) * norm_b, stable sort descending                        bm25.rs:135-170
// The single-query form runs on the host (host/leann_host.hpp, op for op).  A batch of 16 384 queries would spend longer in a host
// rerank than in the traversal, so the same arithmetic — every f32 operation in the same order, IEEE division, no contraction — runs
// here, one workgroup per query, on the lists the traversal kernel left in HBM.  The BM25 side stays what the host's persistent
// Bm25Scorer produces (string / hash work is host work), handed over SPARSE: a BM25 score vector is zero except for
// the passages that share a term with the query, so a query brings its positives (position, score), sorted as Bm25Scorer::search
// sorts them; every other passage scores 0.0 — which is also where min_b comes from whenever fewer than N passages are positive.
// Score polarity: compat_polarity != 0 blends the backend's distances as the reference does (larger distance = larger
// vector term); 0 = corrected, 1 - dist.  Checked bit for bit against oracle/searcher_oracle.py (tests/test_gpu_hybrid.py, bench.py --hybrid).
#include "common.cuh"
#include "../../include/leann_backend.h"
#include "internal.h"

#include "hybrid_rerank.cuh" // the rerank body, shared with the dense-accumulator caller in bm25.hip

__global__ void __launch_bounds__(256) hybrid_rerank_kernel(const uint64_t *__restrict__ keys, const float *__restrict__ dists,
                                                            const uint32_t *__restrict__ counts, uint32_t fetch_k,
                                                            const uint32_t *__restrict__ bm_pos, const float *__restrict__ bm_score,
                                                            const uint32_t *__restrict__ bm_count, uint32_t bm_stride, uint64_t n_docs,
                                                            float alpha, int compat, uint32_t top_k, uint64_t *__restrict__ out_keys,
                                                            float *__restrict__ out_scores, uint32_t *__restrict__ out_counts) {
    const uint32_t q = blockIdx.x;
    // positives beyond the stride are not there to be read: P = min(count, stride)
    const HybSparseBm bm{bm_pos + (size_t)q * bm_stride, bm_score + (size_t)q * bm_stride, min(bm_count[q], bm_stride), n_docs};
    hybrid_rerank_body(bm, keys, dists, counts, fetch_k, alpha, compat, top_k, out_keys, out_scores, out_counts, q);
}

extern "C" int leann_hybrid_rerank_device(const uint64_t *d_keys, const float *d_dists, const uint32_t *d_counts, size_t nq, size_t fetch_k,
                                          const uint32_t *d_bm25_pos, const float *d_bm25_score, const uint32_t *d_bm25_count,
                                          size_t bm25_stride, size_t n_docs, float alpha, int compat_polarity, size_t top_k,
                                          uint64_t *d_out_keys, float *d_out_scores, uint32_t *d_out_counts, void *stream) {
    if (!d_keys || !d_dists || !d_counts || !d_bm25_count || (bm25_stride && (!d_bm25_pos || !d_bm25_score)) || !d_out_keys || !d_out_scores ||
        !d_out_counts || top_k == 0 || fetch_k == 0) {
        leann_set_error("leann_hybrid_rerank_device: null/zero argument");
        return LEANN_ERR_INVALID;
    }
    if (fetch_k > HYB_MAX_FETCH || top_k > HYB_MAX_MERGED) {
        leann_set_error("leann_hybrid_rerank_device: fetch_k %zu > %d (the reference fetches 5 * top_k, searcher.rs:129-133)", fetch_k, HYB_MAX_FETCH);
        return LEANN_ERR_INVALID;
    }
    if (!(alpha >= 0.0f && alpha <= 1.0f)) {
        leann_set_error("leann_hybrid_rerank_device: alpha %g outside [0, 1]", (double)alpha);
        return LEANN_ERR_INVALID;
    }
    if (nq == 0) return LEANN_OK;
    hipLaunchKernelGGL(hybrid_rerank_kernel, dim3((unsigned)nq), dim3(256), 0, (hipStream_t)stream, d_keys, d_dists, d_counts, (uint32_t)fetch_k,
                       d_bm25_pos, d_bm25_score, d_bm25_count, (uint32_t)bm25_stride, (uint64_t)n_docs, alpha, compat_polarity, (uint32_t)top_k,
                       d_out_keys, d_out_scores, d_out_counts);
    HIP_CHECK_RET(hipGetLastError());
    return LEANN_OK;
}
