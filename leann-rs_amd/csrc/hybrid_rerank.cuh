// hybrid_rerank.cuh — the body of the batched hybrid rerank (searcher.rs:146-169 + bm25.rs:135-170), one workgroup of 256 threads per
// query, shared by the two callers that differ only in where a passage's BM25 score comes from:
//   HybSparseBm (hybrid.hip)  the host's Bm25Scorer::search positives, (position, score) pairs, looked up by a linear scan;
//   HybDenseBm  (bm25.hip)    the live accumulator of the device BM25 index, gathered in O(1), with the statistics of the score vector
//                             (positives, min, max over ALL passages) already folded by the selection sweep.
// A policy provides: n_top(fetch_k) = |bm25_top|, top_pos(t) = position of its t-th entry, fold_min_max(...) = the f32::min / f32::max
// folds over the whole BM25 score vector (as orderable u32 in LDS), score(key) = bm25_scores[key] or 0.0 beyond the vector.
#pragma once
#include "common.cuh"

#define HYB_MAX_FETCH 256
#define HYB_MAX_MERGED (2 * HYB_MAX_FETCH)

struct HybSparseBm {
    const uint32_t *bp;
    const float *bs;
    uint32_t P;
    uint64_t n_docs;
    __device__ __forceinline__ uint32_t n_top(uint32_t fetch_k) const { return min(P, fetch_k); } // the first fetch_k positives (searcher.rs:154)
    __device__ __forceinline__ uint64_t top_pos(uint32_t t) const { return bp[t]; }
    __device__ __forceinline__ void fold_min_max(uint32_t tid, uint32_t *s_minb, uint32_t *s_maxb) const {
        for (uint32_t t = tid; t < P; t += 256) {
            const uint32_t o = f32_orderable(bs[t]);
            atomicMin(s_minb, o);
            atomicMax(s_maxb, o);
        }
        if (tid == 0 && (uint64_t)P < n_docs) { // every passage without a term of the query scores 0.0
            const uint32_t z = f32_orderable(0.0f);
            atomicMin(s_minb, z);
            atomicMax(s_maxb, z);
        }
    }
    __device__ __forceinline__ float score(uint64_t key) const {
        float bm = 0.0f; // bm25_scores[idx], 0.0 beyond the vector (bm25.rs:158)
        for (uint32_t t = 0; t < P; t++)
            if ((uint64_t)bp[t] == key) bm = bs[t];
        return bm;
    }
};

struct HybDenseBm {
    const uint64_t *best; // the query's selection keys (~orderable(score) << 32 | position), ascending; the first min(P, fetch_k) are bm25_top
    const float *acc;     // the query's score vector [n_docs]
    uint64_t n_docs;
    uint32_t P, min_o, max_o; // positives, orderable min / max over all n_docs scores
    __device__ __forceinline__ uint32_t n_top(uint32_t fetch_k) const { return min(P, fetch_k); }
    __device__ __forceinline__ uint64_t top_pos(uint32_t t) const { return (uint32_t)best[t]; }
    __device__ __forceinline__ void fold_min_max(uint32_t tid, uint32_t *s_minb, uint32_t *s_maxb) const {
        if (tid == 0) {
            atomicMin(s_minb, min_o);
            atomicMax(s_maxb, max_o);
        }
    }
    __device__ __forceinline__ float score(uint64_t key) const { return key < n_docs ? acc[key] : 0.0f; }
};

template <class Bm>
__device__ __forceinline__ void hybrid_rerank_body(const Bm &bm25, const uint64_t *__restrict__ keys, const float *__restrict__ dists,
                                                   const uint32_t *__restrict__ counts, uint32_t fetch_k, float alpha, int compat,
                                                   uint32_t top_k, uint64_t *__restrict__ out_keys, float *__restrict__ out_scores,
                                                   uint32_t *__restrict__ out_counts, uint32_t q) {
    __shared__ uint64_t m_key[HYB_MAX_MERGED];
    __shared__ float m_v[HYB_MAX_MERGED];
    __shared__ float m_score[HYB_MAX_MERGED];
    __shared__ uint64_t s_sort[HYB_MAX_MERGED];
    __shared__ uint32_t s_inj[HYB_MAX_FETCH];
    __shared__ uint32_t s_minv, s_maxv, s_minb, s_maxb, s_m;
    const uint32_t tid = threadIdx.x;
    const uint32_t n = min(counts[q], fetch_k);
    const uint32_t top = bm25.n_top(fetch_k);
    if (tid == 0) { s_minv = 0xFFFFFFFFu; s_maxv = 0u; s_minb = 0xFFFFFFFFu; s_maxb = 0u; }
    for (uint32_t i = tid; i < n; i += 256) {
        const float d = dists[(size_t)q * fetch_k + i];
        m_key[i] = keys[(size_t)q * fetch_k + i];
        m_v[i] = compat ? d : 1.0f - d;
    }
    __syncthreads();
    // BM25-only hits: positives of bm25_top that the backend did not return, appended in bm25_top order with vector score 0.0
    for (uint32_t t = tid; t < top; t += 256) {
        const uint64_t pos = bm25.top_pos(t);
        uint32_t found = 0;
        for (uint32_t i = 0; i < n; i++) found |= (m_key[i] == pos);
        s_inj[t] = found ? 0u : 1u;
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t m = n;
        for (uint32_t t = 0; t < top; t++)
            if (s_inj[t]) { m_key[m] = bm25.top_pos(t); m_v[m] = 0.0f; m++; }
        s_m = m;
    }
    __syncthreads();
    const uint32_t m = s_m;
    // f32::max / f32::min folds (bm25.rs:140-147, :152-154) — order-independent for non-NaN values
    for (uint32_t i = tid; i < m; i += 256) {
        const uint32_t o = f32_orderable(m_v[i]);
        atomicMin(&s_minv, o);
        atomicMax(&s_maxv, o);
    }
    bm25.fold_min_max(tid, &s_minb, &s_maxb);
    __syncthreads();
    const float min_v = orderable_f32(s_minv), max_v = orderable_f32(s_maxv);
    const float min_b = orderable_f32(s_minb), max_b = orderable_f32(s_maxb);
    const float v_range = fmaxf(max_v - min_v, 1e-6f), b_range = fmaxf(max_b - min_b, 1e-6f);
    const float one_minus_alpha = 1.0f - alpha;
    for (uint32_t i = tid; i < HYB_MAX_MERGED; i += 256) {
        uint64_t sk = ~0ull;
        if (i < m) {
            const float bm = bm25.score(m_key[i]);
            const float norm_vec = (m_v[i] - min_v) / v_range;
            const float norm_b = (bm - min_b) / b_range;
            const float t1 = alpha * norm_vec, t2 = one_minus_alpha * norm_b;
            const float sc = t1 + t2;
            m_score[i] = sc;
            sk = ((uint64_t)(~f32_orderable(sc)) << 32) | i; // ascending = score descending, ties in list order: Rust's stable sort_by
        }
        s_sort[i] = sk;
    }
    int npow = 2;
    while (npow < (int)m) npow <<= 1;
    bitonic_sort_lds(s_sort, npow); // (entries >= m are ~0 and npow <= HYB_MAX_MERGED)
    const uint32_t nout = min(m, top_k);
    for (uint32_t j = tid; j < top_k; j += 256) {
        if (j < nout) {
            const uint32_t i = (uint32_t)s_sort[j];
            out_keys[(size_t)q * top_k + j] = m_key[i];
            out_scores[(size_t)q * top_k + j] = m_score[i];
        } else {
            out_keys[(size_t)q * top_k + j] = ~0ull;
            out_scores[(size_t)q * top_k + j] = -INFINITY;
        }
    }
    if (tid == 0) out_counts[q] = nout;
}
