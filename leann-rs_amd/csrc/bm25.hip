// bm25.hip — Bm25Scorer::score_query + Bm25Scorer::search + the hybrid branch of IndexSearcher::search_with_options for BATCHES of
// queries, from an inverted index that lives in HBM (DESIGN.md "BM25 on the device").
//
// Reference, per query (src/index/bm25.rs:77-122):
//     for token in tokenize(query):                       in query order, a repeated token counts twice (:81), unknown tokens are skipped
//         idf = ln((N - df + 0.5) / (df + 0.5) + 1)       :88 — libm logf on the HOST, handed in with each query term: the device's logf
//                                                          differs in the last bit
//         for every passage with tf > 0:  scores[doc] += idf * (tf * (K1 + 1)) / (tf + K1 * (1 - B + B * (doc_len / avg_doc_len)))
//     search: positives (> 0.0, :115), stable sort descending (:118), truncate
//
// Data: CSR postings (post_doc u32 strictly ascending within a term's list, post_tf u32) and k1n[doc] = K1 * norm(doc), computed once
// with the operations of :97.  A contribution is idf * (tf * (K1 + 1.0f)) / (tf + k1n[doc]): no contraction, IEEE divide (Makefile flags).
//
// Pass structure, for a chunk of at most `slots` queries (one dense f32 accumulator of n_docs entries per slot, zero between calls):
//   score     for token rank j = 0, 1, ...: one launch in which every query of the chunk streams the posting list of its j-th token and
//             does a plain read-add-write.  A list holds a passage once, so within a launch a (slot, passage) pair is touched once; the
//             launches follow each other in the stream: the additions of a passage happen in query-token order, without float atomics.
//             A list is split over up to 2048 workgroups per slot (grid-stride), so a term of a million postings is not one workgroup's.
//   select    a sweep over the accumulators in row ranges that double (8192, 8192, 16384, ...): every score above the query's running
//             k-th best key (fixed for the launch) is appended to the query's candidate list; fold_candidates_kernel (scan.hip) merges the
//             list into the running best-k between launches.  The same sweep counts the positives and folds min / max over ALL n_docs
//             scores (so min_b is 0.0 exactly when a passage is not positive, bm25.rs:152-154).  With passages in no particular order a
//             range brings ~k survivors; a list that overflows (scores rising with the position) sends the chunk to the segment sorter
//             of the exact scan (topk_scores_kernel / topk_keys_kernel / finalize_scan_kernel), which has no such limit.
//   consume   search: best-k -> (position, score) lists;  hybrid: the rerank body of hybrid.hip with the BM25 score of a merged key
//             gathered from the live accumulator.
//   reset     the chunk's accumulators are cleared (one memset node) for the next chunk.
// Under an allow-bitmap (the *_filtered entry points; DESIGN.md §8c "under a filter") scoring is unchanged — idf, doc_len and avg_doc_len
// are the corpus's — and everything after it sees the score vector restricted to the allowed positions: the sweep is
// bm25_emit_masked_kernel, the segment sorter gets the bitmap, and a query that allows nothing is settled by bm25_empty_allow_kernel.
// Without a bitmap the launches are the ones above, the same kernels with the same arguments.
// Selection and reset sweep the dense vector, not the lists: on a Zipf vocabulary a 2-8 term query is positive on nearly every passage,
// where the dense sweep reads 4 B per passage against 12 B per posting, and it needs no claim marks.  The price is 8 B per passage for a
// query with few positives (80 MB = ~16 us at 10M passages).
//
// Slot budget: BM25_ACC_BUDGET = 1 GiB of accumulators -> slots = clamp(1 GiB / (4 B * n_docs), 1, 64): 64 up to 4.19M passages, 26 at 10M.
#include "common.cuh"
#include "../../include/leann_backend.h"
#include "internal.h"
#include "hybrid_rerank.cuh"
#include <algorithm>
#include <cmath>
#include <vector>

#define BM25_ACC_BUDGET ((size_t)1 << 30)
#define BM25_MAX_SLOTS 64
#define BM25_MAX_TOPK 1024 // the fold sorts best-k + survivors in one SEG-wide LDS segment
#define BM25_CAND_CAP 8192 // candidate list per slot; also the first two row ranges, which therefore cannot overflow
#define BM25_MAX_GRID_X 2048

struct Bm25Tok { // one known query token: its posting list and idf
    uint64_t begin;
    uint32_t len;
    float idf;
};

struct leann_bm25 {
    int device = 0;
    size_t n_docs = 0, n_terms = 0, n_post = 0;
    uint32_t slots = 0;
    std::vector<uint64_t> h_off; // post_off, kept on the host: a query token becomes (begin, len) before it is uploaded
    DeviceBuf<uint32_t> d_doc, d_tf;
    DeviceBuf<float> d_k1n, d_acc;                               // acc [slots x n_docs], all zero between calls
    DeviceBuf<uint64_t> d_best, d_list;                          // [slots x BM25_MAX_TOPK], [slots x BM25_CAND_CAP]
    DeviceBuf<float> d_thr;                                      // [slots]
    DeviceBuf<uint32_t> d_cnt, d_stats, d_overflow;              // [slots], [slots x 4] {P, min, max, allowed rows (masked sweep)}, [1]
    uint32_t *h_overflow = nullptr;                              // pinned
    DeviceBuf<Bm25Tok> d_toks;                                   // query tokens / offsets of the running batch; grown, never shrunk
    DeviceBuf<uint32_t> d_qoff;
    std::mutex mu;                                               // one batch at a time owns the accumulators
};

static constexpr float BM25_K1 = 1.2f, BM25_B = 0.75f; // bm25.rs:9-10

// ------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) bm25_score_pass_kernel(const Bm25Tok *__restrict__ toks, const uint32_t *__restrict__ q_off, uint32_t q0,
                                                              uint32_t rank, const uint32_t *__restrict__ post_doc,
                                                              const uint32_t *__restrict__ post_tf, const float *__restrict__ k1n,
                                                              float *__restrict__ acc, uint64_t n_docs) {
    const uint32_t slot = blockIdx.y;
    const uint32_t t0 = q_off[q0 + slot], t1 = q_off[q0 + slot + 1];
    if (t1 - t0 <= rank) return;
    const Bm25Tok tk = toks[t0 + rank];
    const uint32_t *__restrict__ pd = post_doc + tk.begin;
    const uint32_t *__restrict__ pt = post_tf + tk.begin;
    float *__restrict__ a = acc + (size_t)slot * n_docs;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < tk.len; i += gridDim.x * 256u) {
        const uint32_t doc = pd[i];
        const float tf = (float)pt[i];
        if (doc >= n_docs) continue; // validated at creation; never taken
        const float score = tk.idf * (tf * (BM25_K1 + 1.0f)) / (tf + k1n[doc]); // bm25.rs:100
        a[doc] = a[doc] + score;
    }
}

__global__ void bm25_select_init_kernel(uint64_t *__restrict__ best, uint32_t k, float *__restrict__ thr, uint32_t *__restrict__ cnt,
                                        uint32_t *__restrict__ stats, uint32_t *__restrict__ overflow) {
    const uint32_t slot = blockIdx.x;
    for (uint32_t i = threadIdx.x; i < k; i += blockDim.x) best[(size_t)slot * k + i] = ~0ull;
    if (threadIdx.x == 0) {
        thr[slot] = __uint_as_float(0xFF800000u); // -inf: fewer than k so far
        cnt[slot] = 0;
        stats[slot * 4 + 0] = 0;
        stats[slot * 4 + 1] = 0xFFFFFFFFu;
        stats[slot * 4 + 2] = 0;
        stats[slot * 4 + 3] = 0;
        if (slot == 0) *overflow = 0;
    }
}

// rows [r0, r1) of every slot's accumulator: count positives, fold min / max, append the scores that can still enter the best-k
__global__ void __launch_bounds__(256) bm25_emit_kernel(const float *__restrict__ acc, uint64_t n_docs, uint32_t r0, uint32_t r1,
                                                        const uint64_t *__restrict__ best, uint32_t k, uint32_t *__restrict__ cnt,
                                                        uint64_t *__restrict__ list, uint32_t cap, uint32_t *__restrict__ stats) {
    __shared__ uint32_t s_p, s_min, s_max;
    const uint32_t slot = blockIdx.y;
    const float *__restrict__ a = acc + (size_t)slot * n_docs;
    const uint64_t bound = best[(size_t)slot * k + (k - 1)]; // the running k-th best key (~0: fewer than k so far), fixed for the launch
    if (threadIdx.x == 0) { s_p = 0; s_min = 0xFFFFFFFFu; s_max = 0; }
    __syncthreads();
    uint32_t p = 0, mn = 0xFFFFFFFFu, mx = 0;
    for (uint32_t row = r0 + blockIdx.x * 256u + threadIdx.x; row < r1; row += gridDim.x * 256u) {
        const float v = a[row];
        const uint32_t o = f32_orderable(v);
        mn = min(mn, o);
        mx = max(mx, o);
        if (v > 0.0f) { // bm25.rs:115
            p++;
            const uint64_t key = ((uint64_t)(~o) << 32) | row;
            if (key < bound) { // keys are unique and order (score desc, position asc): a tie with the k-th best at a later position is out
                const uint32_t at = atomicAdd(&cnt[slot], 1u);
                if (at < cap) list[(size_t)slot * cap + at] = key;
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        p += __shfl_xor(p, off);
        mn = min(mn, (uint32_t)__shfl_xor(mn, off));
        mx = max(mx, (uint32_t)__shfl_xor(mx, off));
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&s_p, p);
        atomicMin(&s_min, mn);
        atomicMax(&s_max, mx);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_p) atomicAdd(&stats[slot * 4 + 0], s_p);
        atomicMin(&stats[slot * 4 + 1], s_min);
        atomicMax(&stats[slot * 4 + 2], s_max);
    }
}

// bm25_emit_kernel under an allow-bitmap (bit row & 7 of byte row >> 3): a row whose bit is clear contributes to nothing — not to the
// positives, not to min / max, not to the candidate list — and stats[slot * 4 + 3] counts the allowed rows, so that the consumers can
// tell an empty allowed set (whose min / max have no orderable encoding) from any other.  The slot's bitmap is allow + slot *
// allow_stride (the caller has added the chunk's q0 * allow_stride).  Every launch starts at a multiple of BM25_CAND_CAP rows and a
// workgroup's 256 rows at a multiple of 256, so each aligned group of 32 lanes covers the rows of one 4-byte group of the bitmap: its
// first lane reads the bytes (singly: a stride need not be a multiple of 4, and no byte behind ceil(n_docs / 8) is touched) and the
// other 31 take the word by a shuffle.  4 bitmap bytes per 128 bytes of scores.  Every lane asks for its score before the word is there.
__global__ void __launch_bounds__(256) bm25_emit_masked_kernel(const float *__restrict__ acc, uint64_t n_docs, uint32_t r0, uint32_t r1,
                                                               const uint64_t *__restrict__ best, uint32_t k, uint32_t *__restrict__ cnt,
                                                               uint64_t *__restrict__ list, uint32_t cap, uint32_t *__restrict__ stats,
                                                               const uint8_t *__restrict__ allow, uint64_t allow_stride) {
    __shared__ uint32_t s_p, s_min, s_max, s_a;
    const uint32_t slot = blockIdx.y;
    const float *__restrict__ a = acc + (size_t)slot * n_docs;
    const uint8_t *__restrict__ bits = allow + (size_t)slot * allow_stride;
    const uint32_t nbytes = (uint32_t)((n_docs + 7) >> 3);
    const uint64_t bound = best[(size_t)slot * k + (k - 1)];
    if (threadIdx.x == 0) { s_p = 0; s_min = 0xFFFFFFFFu; s_max = 0; s_a = 0; }
    __syncthreads();
    uint32_t p = 0, mn = 0xFFFFFFFFu, mx = 0, na = 0;
    const uint32_t lane = threadIdx.x & 63;
    for (uint32_t base = r0 + blockIdx.x * 256u; base < r1; base += gridDim.x * 256u) { // uniform over the workgroup: every lane shuffles
        const uint32_t row = base + threadIdx.x;
        const bool in = row < r1;
        const float v = in ? a[row] : 0.0f; // asked for beside the bitmap bytes, not behind them: one memory latency per step, not two
        uint32_t w = 0;
        if ((lane & 31) == 0 && in) {
            const uint32_t b0 = row >> 3; // row is a multiple of 32 here
            if (b0 + 3 < nbytes) {
                w = (uint32_t)bits[b0] | ((uint32_t)bits[b0 + 1] << 8) | ((uint32_t)bits[b0 + 2] << 16) | ((uint32_t)bits[b0 + 3] << 24);
            } else { // the bitmap's last bytes
                for (uint32_t i = 0; i < 4; i++)
                    if (b0 + i < nbytes) w |= (uint32_t)bits[b0 + i] << (8 * i);
            }
        }
        w = __shfl(w, (int)(lane & 32));
        if (in && ((w >> (lane & 31)) & 1)) {
            na++;
            const uint32_t o = f32_orderable(v);
            mn = min(mn, o);
            mx = max(mx, o);
            if (v > 0.0f) {
                p++;
                const uint64_t key = ((uint64_t)(~o) << 32) | row;
                if (key < bound) {
                    const uint32_t at = atomicAdd(&cnt[slot], 1u);
                    if (at < cap) list[(size_t)slot * cap + at] = key;
                }
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        p += __shfl_xor(p, off);
        na += __shfl_xor(na, off);
        mn = min(mn, (uint32_t)__shfl_xor(mn, off));
        mx = max(mx, (uint32_t)__shfl_xor(mx, off));
    }
    if (lane == 0) {
        atomicAdd(&s_p, p);
        atomicAdd(&s_a, na);
        atomicMin(&s_min, mn);
        atomicMax(&s_max, mx);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_p) atomicAdd(&stats[slot * 4 + 0], s_p);
        if (s_a) atomicAdd(&stats[slot * 4 + 3], s_a);
        atomicMin(&stats[slot * 4 + 1], s_min);
        atomicMax(&stats[slot * 4 + 2], s_max);
    }
}

// overflow path: (position, score) lists of the segment sorter -> selection keys; rows that are not positive sort last and are cut
__global__ void bm25_rebuild_best_kernel(const uint64_t *__restrict__ keys, const float *__restrict__ scores, uint32_t k,
                                         uint64_t *__restrict__ best) {
    const uint32_t slot = blockIdx.x;
    for (uint32_t i = threadIdx.x; i < k; i += blockDim.x) {
        const uint64_t key = keys[(size_t)slot * k + i];
        const float sc = scores[(size_t)slot * k + i];
        best[(size_t)slot * k + i] = (key != ~0ull && sc > 0.0f) ? (((uint64_t)(~f32_orderable(sc)) << 32) | (uint32_t)key) : ~0ull;
    }
}

__global__ void bm25_finalize_kernel(const uint64_t *__restrict__ best, const uint32_t *__restrict__ stats, uint32_t k,
                                     uint32_t *__restrict__ pos, float *__restrict__ scores, uint32_t *__restrict__ counts,
                                     uint32_t *__restrict__ n_positive, float *__restrict__ min_max) {
    const uint32_t q = blockIdx.x; // pointers are already at the chunk's first query
    const uint32_t P = stats[q * 4 + 0];
    const uint32_t n = min(P, k);
    for (uint32_t i = threadIdx.x; i < k; i += blockDim.x) {
        const uint64_t key = best[(size_t)q * k + i];
        const bool ok = i < n && key != ~0ull;
        pos[(size_t)q * k + i] = ok ? (uint32_t)key : 0xFFFFFFFFu;
        scores[(size_t)q * k + i] = ok ? orderable_f32(~(uint32_t)(key >> 32)) : __uint_as_float(0xFF800000u);
    }
    if (threadIdx.x == 0) {
        counts[q] = n;
        if (n_positive) n_positive[q] = P;
        if (min_max) {
            min_max[q * 2 + 0] = orderable_f32(stats[q * 4 + 1]);
            min_max[q * 2 + 1] = orderable_f32(stats[q * 4 + 2]);
        }
    }
}

__global__ void __launch_bounds__(256) bm25_hybrid_rerank_kernel(const uint64_t *__restrict__ keys, const float *__restrict__ dists,
                                                                 const uint32_t *__restrict__ counts, uint32_t fetch_k,
                                                                 const uint64_t *__restrict__ best, const float *__restrict__ acc,
                                                                 const uint32_t *__restrict__ stats, uint64_t n_docs, float alpha, int compat,
                                                                 uint32_t top_k, uint64_t *__restrict__ out_keys,
                                                                 float *__restrict__ out_scores, uint32_t *__restrict__ out_counts) {
    const uint32_t q = blockIdx.x; // slot == query within the chunk
    const HybDenseBm bm{best + (size_t)q * fetch_k, acc + (size_t)q * n_docs, n_docs, stats[q * 4 + 0], stats[q * 4 + 1], stats[q * 4 + 2]};
    hybrid_rerank_body(bm, keys, dists, counts, fetch_k, alpha, compat, top_k, out_keys, out_scores, out_counts, q);
}

// After the consumer of a masked chunk: a query whose bitmap allows no position.  Its folds never ran, and their identities (+inf,
// -inf) are not what the orderable sentinels of d_stats decode to, so they are written here; the rerank of such a query returns
// nothing whatever its ANN list holds.  (The search consumer has written count 0, n_positive 0 and the tails already: P == 0.)
__global__ void bm25_empty_allow_kernel(const uint32_t *__restrict__ stats, float *__restrict__ min_max, uint32_t top_k,
                                        uint64_t *__restrict__ out_keys, float *__restrict__ out_scores, uint32_t *__restrict__ out_counts) {
    const uint32_t q = blockIdx.x; // pointers are already at the chunk's first query
    if (stats[q * 4 + 3] != 0) return;
    if (min_max && threadIdx.x == 0) {
        min_max[q * 2 + 0] = __uint_as_float(0x7F800000u);
        min_max[q * 2 + 1] = __uint_as_float(0xFF800000u);
    }
    if (out_keys) {
        for (uint32_t j = threadIdx.x; j < top_k; j += blockDim.x) {
            out_keys[(size_t)q * top_k + j] = ~0ull;
            out_scores[(size_t)q * top_k + j] = __uint_as_float(0xFF800000u);
        }
        if (threadIdx.x == 0) out_counts[q] = 0;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// validation (host only: works without a device)
extern "C" int leann_bm25_check_queries(size_t n_terms, size_t nq, const uint32_t *q_off, const uint32_t *q_term, const float *q_idf) {
    if (nq == 0) return LEANN_OK;
    if (!q_off) {
        leann_set_error("leann_bm25: null q_off");
        return LEANN_ERR_INVALID;
    }
    if (nq >= 0xFFFFFFFFull) {
        leann_set_error("leann_bm25: nq %zu too large", nq);
        return LEANN_ERR_INVALID;
    }
    if (q_off[0] != 0) {
        leann_set_error("leann_bm25: q_off[0] = %u, expected 0", q_off[0]);
        return LEANN_ERR_INVALID;
    }
    for (size_t i = 0; i < nq; i++)
        if (q_off[i + 1] < q_off[i]) {
            leann_set_error("leann_bm25: q_off not monotone at query %zu (%u > %u)", i, q_off[i], q_off[i + 1]);
            return LEANN_ERR_INVALID;
        }
    const size_t nt = q_off[nq];
    if (nt && (!q_term || !q_idf)) {
        leann_set_error("leann_bm25: null q_term / q_idf");
        return LEANN_ERR_INVALID;
    }
    for (size_t t = 0; t < nt; t++) {
        if (q_term[t] >= n_terms) {
            leann_set_error("leann_bm25: q_term[%zu] = %u >= n_terms %zu", t, q_term[t], n_terms);
            return LEANN_ERR_INVALID;
        }
        if (!(q_idf[t] >= 0.0f) || std::isinf(q_idf[t])) { // ln(x + 1) with x > 0 (bm25.rs:88) is never negative
            leann_set_error("leann_bm25: q_idf[%zu] = %g is negative or not finite", t, (double)q_idf[t]);
            return LEANN_ERR_INVALID;
        }
    }
    return LEANN_OK;
}

static void bm25_free(leann_bm25 *b) {
    if (!b) return;
    int prev = 0;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(b->device); // the owning device is current while `delete b` frees the handle's buffers
    if (b->h_overflow) (void)hipHostFree(b->h_overflow);
    delete b;
    (void)hipSetDevice(prev);
}

extern "C" int leann_bm25_create(size_t n_docs, size_t n_terms, const uint64_t *post_off, const uint32_t *post_doc, const uint32_t *post_tf,
                                 const uint32_t *doc_len, float avg_doc_len, int device, leann_bm25 **out) {
    if (!out) {
        leann_set_error("leann_bm25_create: null out");
        return LEANN_ERR_INVALID;
    }
    *out = nullptr;
    if (!post_off || !doc_len) {
        leann_set_error("leann_bm25_create: null post_off / doc_len");
        return LEANN_ERR_INVALID;
    }
    if (n_docs == 0 || n_docs > 0x7FFFFFFFull) {
        leann_set_error("leann_bm25_create: n_docs %zu outside [1, 2^31)", n_docs);
        return LEANN_ERR_INVALID;
    }
    if (n_terms > 0xFFFFFFFFull) {
        leann_set_error("leann_bm25_create: n_terms %zu does not fit a u32 term id", n_terms);
        return LEANN_ERR_INVALID;
    }
    if (!(avg_doc_len > 0.0f) || std::isinf(avg_doc_len)) {
        leann_set_error("leann_bm25_create: avg_doc_len %g is not a positive finite number", (double)avg_doc_len);
        return LEANN_ERR_INVALID;
    }
    if (post_off[0] != 0) {
        leann_set_error("leann_bm25_create: post_off[0] = %llu, expected 0", (unsigned long long)post_off[0]);
        return LEANN_ERR_INVALID;
    }
    for (size_t t = 0; t < n_terms; t++) {
        if (post_off[t + 1] < post_off[t]) {
            leann_set_error("leann_bm25_create: post_off not monotone at term %zu", t);
            return LEANN_ERR_INVALID;
        }
        if (post_off[t + 1] - post_off[t] > n_docs) {
            leann_set_error("leann_bm25_create: post_off gives term %zu more postings than there are passages", t);
            return LEANN_ERR_INVALID;
        }
    }
    const size_t n_post = post_off[n_terms];
    if (n_post && (!post_doc || !post_tf)) {
        leann_set_error("leann_bm25_create: null post_doc / post_tf");
        return LEANN_ERR_INVALID;
    }
    for (size_t t = 0; t < n_terms; t++)
        for (uint64_t i = post_off[t]; i < post_off[t + 1]; i++) {
            if (post_doc[i] >= n_docs) {
                leann_set_error("leann_bm25_create: post_doc[%llu] = %u >= n_docs %zu", (unsigned long long)i, post_doc[i], n_docs);
                return LEANN_ERR_INVALID;
            }
            if (i > post_off[t] && post_doc[i] <= post_doc[i - 1]) {
                leann_set_error("leann_bm25_create: post_doc out of order at %llu (term %zu): passages of a list must ascend strictly",
                                (unsigned long long)i, t);
                return LEANN_ERR_INVALID;
            }
            if (post_tf[i] == 0) {
                leann_set_error("leann_bm25_create: post_tf[%llu] = 0 (tf == 0 is not a posting)", (unsigned long long)i);
                return LEANN_ERR_INVALID;
            }
        }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        (void)hipGetLastError();
        leann_set_error("leann_bm25_create: no HIP device visible (this library has no CPU fallback)");
        return LEANN_ERR_DEVICE;
    }
    if (device < 0 || device >= ndev) {
        leann_set_error("leann_bm25_create: device %d outside [0, %d)", device, ndev);
        return LEANN_ERR_INVALID;
    }
    std::vector<float> k1n(n_docs);
    for (size_t i = 0; i < n_docs; i++) {
        const float dl = (float)doc_len[i];
        const float norm = 1.0f - BM25_B + BM25_B * (dl / avg_doc_len); // bm25.rs:97
        k1n[i] = BM25_K1 * norm;                                          // :100, the denominator's second term
    }
    int prev = 0;
    HIP_CHECK_RET(hipGetDevice(&prev));
    HIP_CHECK_RET(hipSetDevice(device));
    leann_bm25 *b = new leann_bm25;
    b->device = device;
    b->n_docs = n_docs;
    b->n_terms = n_terms;
    b->n_post = n_post;
    b->h_off.assign(post_off, post_off + n_terms + 1);
    b->slots = (uint32_t)std::min<size_t>(BM25_MAX_SLOTS, std::max<size_t>(1, BM25_ACC_BUDGET / (sizeof(float) * n_docs)));
    const size_t S = b->slots;
    hipError_t e = hipSuccess;
    auto alloc = [&](auto &buf, size_t count) { // (256 bytes at the least)
        if (e == hipSuccess && buf.alloc(std::max<size_t>(count, 256 / sizeof(*buf.p)))) e = hipErrorOutOfMemory;
    };
    alloc(b->d_doc, n_post);
    alloc(b->d_tf, n_post);
    alloc(b->d_k1n, n_docs);
    alloc(b->d_acc, S * n_docs);
    alloc(b->d_best, S * BM25_MAX_TOPK);
    alloc(b->d_list, S * BM25_CAND_CAP);
    alloc(b->d_thr, S);
    alloc(b->d_cnt, S);
    alloc(b->d_stats, S * 4);
    alloc(b->d_overflow, 1);
    if (e == hipSuccess) e = hipHostMalloc((void **)&b->h_overflow, 4, hipHostMallocDefault);
    if (e == hipSuccess && n_post) e = hipMemcpy(b->d_doc, post_doc, n_post * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && n_post) e = hipMemcpy(b->d_tf, post_tf, n_post * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(b->d_k1n, k1n.data(), n_docs * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(b->d_acc, 0, S * n_docs * 4);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    (void)hipSetDevice(prev);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        bm25_free(b);
        leann_set_error("leann_bm25_create: %s", hipGetErrorString(e));
        return LEANN_ERR_DEVICE;
    }
    *out = b;
    return LEANN_OK;
}

extern "C" size_t leann_bm25_len(const leann_bm25 *b) { return b ? b->n_docs : 0; }
extern "C" size_t leann_bm25_slots(const leann_bm25 *b) { return b ? b->slots : 0; }
extern "C" void leann_bm25_close(leann_bm25 *b) { bm25_free(b); }

// ------------------------------------------------------------------------------------------------------------------------------------
struct Bm25Consumer { // what happens to a chunk's best-k while its accumulators are live; output pointers are for the whole batch
    bool hybrid = false;
    // search
    uint32_t *d_pos = nullptr, *d_counts = nullptr, *d_npos = nullptr;
    float *d_scores = nullptr, *d_minmax = nullptr;
    // hybrid
    const uint64_t *d_keys = nullptr;
    const float *d_dists = nullptr;
    const uint32_t *d_vcounts = nullptr;
    float alpha = 0.0f;
    int compat = 1;
    uint32_t top_k = 0;
    uint64_t *d_out_keys = nullptr;
    float *d_out_scores = nullptr;
    uint32_t *d_out_counts = nullptr;
    // both: an allow-bitmap on the handle's device (null: none), query i's at d_allow + i * allow_stride
    const uint8_t *d_allow = nullptr;
    size_t allow_stride = 0;
};

// best-k of the chunk's nslots accumulators by the segment sorter of the exact scan (no list to overflow)
// `allow`: the bitmap of the chunk's first slot (null: none); with a stride the slots are sorted one by one, each under its own
static int bm25_select_by_segments(leann_bm25 *b, uint32_t nslots, uint32_t k, const uint8_t *allow, size_t allow_stride, hipStream_t st) {
    const size_t segs = (b->n_docs + SEG - 1) / SEG, cand_len = segs * k;
    DeviceBuf<uint64_t> candA, candB, keys;
    DeviceBuf<float> scores;
    DeviceBuf<uint32_t> counts;
    if (candA.alloc(nslots * cand_len) || candB.alloc(nslots * cand_len) || keys.alloc((size_t)nslots * k) || scores.alloc((size_t)nslots * k) ||
        counts.alloc(nslots))
        return LEANN_ERR_DEVICE;
    size_t segs_out = 0;
    int rc = LEANN_OK;
    if (allow && allow_stride) {
        for (uint32_t s = 0; s < nslots && rc == LEANN_OK; s++)
            rc = leann_internal_topk_chunk(b->d_acc + (size_t)s * b->n_docs, b->n_docs, 1, k, allow + (size_t)s * allow_stride, 0,
                                           candA + (size_t)s * cand_len, cand_len, 0, st, &segs_out, nullptr);
    } else {
        rc = leann_internal_topk_chunk(b->d_acc, b->n_docs, nslots, k, allow, 0, candA, cand_len, 0, st, &segs_out, nullptr);
    }
    if (rc == LEANN_OK) rc = leann_internal_scan_finish_ex(candA, candB, cand_len, segs_out, nslots, k, 0, keys, scores, counts, st, nullptr, 0);
    if (rc == LEANN_OK) {
        hipLaunchKernelGGL(bm25_rebuild_best_kernel, dim3(nslots), dim3(256), 0, st, keys.p, scores.p, k, b->d_best.p);
        if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) {
            leann_set_error("leann_bm25: segment selection failed on the device");
            rc = LEANN_ERR_DEVICE;
        }
    }
    return rc;
}

static int bm25_run(leann_bm25 *b, size_t nq, const uint32_t *q_off, const uint32_t *q_term, const float *q_idf, uint32_t k,
                    const Bm25Consumer &c, hipStream_t st) {
    std::lock_guard<std::mutex> lk(b->mu);
    int prev = 0;
    HIP_CHECK_RET(hipGetDevice(&prev));
    HIP_CHECK_RET(hipSetDevice(b->device));
    const size_t nt = q_off[nq];
    std::vector<Bm25Tok> toks(std::max<size_t>(nt, 1));
    for (size_t t = 0; t < nt; t++) {
        const uint64_t lo = b->h_off[q_term[t]], hi = b->h_off[q_term[t] + 1];
        toks[t] = Bm25Tok{lo, (uint32_t)(hi - lo), q_idf[t]};
    }
    int rc = LEANN_OK;
    auto fail = [&](hipError_t e, const char *what) {
        if (e == hipSuccess || rc != LEANN_OK) return;
        (void)hipGetLastError();
        leann_set_error("leann_bm25: %s failed: %s", what, hipGetErrorString(e));
        rc = LEANN_ERR_DEVICE;
    };
    if (b->d_toks.cap < toks.size()) rc = b->d_toks.grow(toks.size() * 2); // twice what is needed: headroom for the next batch
    if (rc == LEANN_OK && b->d_qoff.cap < nq + 1) rc = b->d_qoff.grow((nq + 1) * 2);
    Bm25Tok *d_toks = b->d_toks;
    uint32_t *d_qoff = b->d_qoff;
    if (rc == LEANN_OK) fail(hipMemcpy(d_toks, toks.data(), toks.size() * sizeof(Bm25Tok), hipMemcpyHostToDevice), "hipMemcpy");
    if (rc == LEANN_OK) fail(hipMemcpy(d_qoff, q_off, (nq + 1) * 4, hipMemcpyHostToDevice), "hipMemcpy");
    const uint32_t n_docs32 = (uint32_t)b->n_docs;
    for (size_t q0 = 0; q0 < nq && rc == LEANN_OK; q0 += b->slots) {
        const uint32_t ns = (uint32_t)std::min<size_t>(b->slots, nq - q0);
        // score: one launch per token rank, sized by the longest list of that rank
        uint32_t max_rank = 0;
        for (uint32_t s = 0; s < ns; s++) max_rank = std::max(max_rank, q_off[q0 + s + 1] - q_off[q0 + s]);
        for (uint32_t j = 0; j < max_rank; j++) {
            uint32_t longest = 0;
            for (uint32_t s = 0; s < ns; s++)
                if (q_off[q0 + s + 1] - q_off[q0 + s] > j) longest = std::max(longest, toks[q_off[q0 + s] + j].len);
            if (!longest) continue;
            const unsigned gx = (unsigned)std::min<size_t>(BM25_MAX_GRID_X, ((size_t)longest + 1023) / 1024);
            hipLaunchKernelGGL(bm25_score_pass_kernel, dim3(gx, ns), dim3(256), 0, st, d_toks, d_qoff, (uint32_t)q0, j, b->d_doc, b->d_tf,
                               b->d_k1n, b->d_acc, (uint64_t)b->n_docs);
        }
        // select
        const uint8_t *allow = c.d_allow ? c.d_allow + q0 * c.allow_stride : nullptr; // the bitmap of the chunk's first query
        hipLaunchKernelGGL(bm25_select_init_kernel, dim3(ns), dim3(256), 0, st, b->d_best, k, b->d_thr, b->d_cnt, b->d_stats, b->d_overflow);
        CandEmit em{b->d_thr, b->d_cnt, b->d_list, BM25_CAND_CAP, nullptr, 0};
        for (uint32_t r0 = 0, len = BM25_CAND_CAP; r0 < n_docs32 && rc == LEANN_OK;) {
            const uint32_t r1 = (uint32_t)std::min<uint64_t>((uint64_t)r0 + len, n_docs32);
            const unsigned gx = (unsigned)std::min<size_t>(BM25_MAX_GRID_X, ((size_t)(r1 - r0) + 1023) / 1024);
            if (allow)
                hipLaunchKernelGGL(bm25_emit_masked_kernel, dim3(gx, ns), dim3(256), 0, st, b->d_acc, (uint64_t)b->n_docs, r0, r1, b->d_best, k,
                                   b->d_cnt, b->d_list, (uint32_t)BM25_CAND_CAP, b->d_stats, allow, (uint64_t)c.allow_stride);
            else
                hipLaunchKernelGGL(bm25_emit_kernel, dim3(gx, ns), dim3(256), 0, st, b->d_acc, (uint64_t)b->n_docs, r0, r1, b->d_best, k, b->d_cnt,
                                   b->d_list, (uint32_t)BM25_CAND_CAP, b->d_stats);
            rc = leann_internal_fold_candidates(em, k, ns, ns, b->d_best, b->d_overflow, st);
            r0 = r1;
            len = r0; // the next range doubles the rows seen: ~k survivors per range whatever its length
        }
        if (rc != LEANN_OK) break;
        fail(hipMemcpyAsync(b->h_overflow, b->d_overflow, 4, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
        fail(hipStreamSynchronize(st), "hipStreamSynchronize");
        if (rc != LEANN_OK) break;
        if (*b->h_overflow) {
            leann_log(LEANN_LOG_DEBUG, "bm25: a candidate list overflowed, chunk at query %zu selects by segments", q0);
            rc = bm25_select_by_segments(b, ns, k, allow, c.allow_stride, st);
            if (rc != LEANN_OK) break;
        }
        // consume
        if (c.hybrid) {
            hipLaunchKernelGGL(bm25_hybrid_rerank_kernel, dim3(ns), dim3(256), 0, st, c.d_keys + q0 * k, c.d_dists + q0 * k, c.d_vcounts + q0, k,
                               b->d_best, b->d_acc, b->d_stats, (uint64_t)b->n_docs, c.alpha, c.compat, c.top_k, c.d_out_keys + q0 * c.top_k,
                               c.d_out_scores + q0 * c.top_k, c.d_out_counts + q0);
        } else {
            hipLaunchKernelGGL(bm25_finalize_kernel, dim3(ns), dim3(256), 0, st, b->d_best, b->d_stats, k, c.d_pos + q0 * k, c.d_scores + q0 * k,
                               c.d_counts + q0, c.d_npos ? c.d_npos + q0 : nullptr, c.d_minmax ? c.d_minmax + q0 * 2 : nullptr);
        }
        if (allow)
            hipLaunchKernelGGL(bm25_empty_allow_kernel, dim3(ns), dim3(256), 0, st, b->d_stats, c.d_minmax ? c.d_minmax + q0 * 2 : nullptr, c.top_k,
                               c.hybrid ? c.d_out_keys + q0 * c.top_k : nullptr, c.hybrid ? c.d_out_scores + q0 * c.top_k : nullptr,
                               c.hybrid ? c.d_out_counts + q0 : nullptr);
        // reset
        fail(hipMemsetAsync(b->d_acc, 0, (size_t)ns * b->n_docs * 4, st), "hipMemsetAsync");
        fail(hipGetLastError(), "kernel launch");
    }
    // the batch owns the accumulators until its last reset has run
    {
        const hipError_t e = hipStreamSynchronize(st);
        if (rc == LEANN_OK) fail(e, "hipStreamSynchronize");
        else if (b->d_acc) { (void)hipMemset(b->d_acc, 0, (size_t)b->slots * b->n_docs * 4); (void)hipGetLastError(); }
    }
    (void)hipSetDevice(prev);
    return rc;
}

static int bm25_check_search(const char *fn, const leann_bm25 *b, size_t nq, const uint32_t *q_off, const uint32_t *q_term, const float *q_idf,
                             size_t top_k) {
    if (top_k == 0 || top_k > BM25_MAX_TOPK) {
        leann_set_error("%s: top_k %zu outside [1, %d]", fn, top_k, BM25_MAX_TOPK);
        return LEANN_ERR_INVALID;
    }
    if (nq && !q_off) {
        leann_set_error("%s: null q_off", fn);
        return LEANN_ERR_INVALID;
    }
    if (!b) { // the term ids below are checked against the handle's vocabulary
        const int rc = leann_bm25_check_queries((size_t)-1, nq, q_off, q_term, q_idf);
        if (rc != LEANN_OK) return rc;
        leann_set_error("%s: null handle", fn);
        return LEANN_ERR_INVALID;
    }
    return leann_bm25_check_queries(b->n_terms, nq, q_off, q_term, q_idf);
}

// the bitmap arguments of the *_filtered calls; a null handle is reported by the query checks that follow
static int bm25_check_allow(const char *fn, const leann_bm25 *b, const void *allow, size_t allow_stride) {
    if (!allow && allow_stride) {
        leann_set_error("%s: allow is null but allow_stride is %zu (no bitmap means stride 0)", fn, allow_stride);
        return LEANN_ERR_INVALID;
    }
    if (b && allow && allow_stride && allow_stride < (b->n_docs + 7) / 8) {
        leann_set_error("%s: allow_stride %zu is smaller than the %zu-byte bitmap of %zu passages", fn, allow_stride, (b->n_docs + 7) / 8,
                        b->n_docs);
        return LEANN_ERR_INVALID;
    }
    return LEANN_OK;
}

static int bm25_search_device(const char *fn, const leann_bm25 *b, size_t nq, const uint32_t *q_off, const uint32_t *q_term, const float *q_idf,
                              size_t top_k, const uint8_t *d_allow, size_t allow_stride, uint32_t *d_pos, float *d_scores, uint32_t *d_counts,
                              uint32_t *d_n_positive, float *d_min_max, void *stream) {
    int rc = bm25_check_allow(fn, b, d_allow, allow_stride);
    if (rc == LEANN_OK) rc = bm25_check_search(fn, b, nq, q_off, q_term, q_idf, top_k);
    if (rc != LEANN_OK) return rc;
    if (nq == 0) return LEANN_OK;
    if (!d_pos || !d_scores || !d_counts) {
        leann_set_error("%s: null output", fn);
        return LEANN_ERR_INVALID;
    }
    Bm25Consumer c;
    c.d_pos = d_pos; c.d_scores = d_scores; c.d_counts = d_counts; c.d_npos = d_n_positive; c.d_minmax = d_min_max;
    c.d_allow = d_allow; c.allow_stride = allow_stride;
    return bm25_run(const_cast<leann_bm25 *>(b), nq, q_off, q_term, q_idf, (uint32_t)top_k, c, (hipStream_t)stream);
}

extern "C" int leann_bm25_search_batch_device(const leann_bm25 *b, size_t nq, const uint32_t *q_off, const uint32_t *q_term, const float *q_idf,
                                              size_t top_k, uint32_t *d_pos, float *d_scores, uint32_t *d_counts, uint32_t *d_n_positive,
                                              float *d_min_max, void *stream) {
    return bm25_search_device("leann_bm25_search_batch_device", b, nq, q_off, q_term, q_idf, top_k, nullptr, 0, d_pos, d_scores, d_counts,
                              d_n_positive, d_min_max, stream);
}

extern "C" int leann_bm25_search_filtered_batch_device(const leann_bm25 *b, size_t nq, const uint32_t *q_off, const uint32_t *q_term,
                                                       const float *q_idf, size_t top_k, const uint8_t *d_allow, size_t allow_stride,
                                                       uint32_t *d_pos, float *d_scores, uint32_t *d_counts, uint32_t *d_n_positive,
                                                       float *d_min_max, void *stream) {
    return bm25_search_device("leann_bm25_search_filtered_batch_device", b, nq, q_off, q_term, q_idf, top_k, d_allow, allow_stride, d_pos,
                              d_scores, d_counts, d_n_positive, d_min_max, stream);
}

static int bm25_search_host(const char *fn, const leann_bm25 *b, size_t nq, const uint32_t *q_off, const uint32_t *q_term, const float *q_idf,
                            size_t top_k, const uint8_t *allow, size_t allow_stride, uint32_t *pos, float *scores, uint32_t *counts,
                            uint32_t *n_positive, float *min_max) {
    int rc = bm25_check_allow(fn, b, allow, allow_stride);
    if (rc == LEANN_OK) rc = bm25_check_search(fn, b, nq, q_off, q_term, q_idf, top_k);
    if (rc != LEANN_OK) return rc;
    if (nq == 0) return LEANN_OK;
    if (!pos || !scores || !counts) {
        leann_set_error("%s: null output", fn);
        return LEANN_ERR_INVALID;
    }
    int prev = 0;
    HIP_CHECK_RET(hipGetDevice(&prev));
    HIP_CHECK_RET(hipSetDevice(b->device));
    DeviceBuf<unsigned char> d;
    const size_t nbytes = (b->n_docs + 7) / 8; // of one bitmap; the last query's need not be followed by a whole stride
    const size_t allow_bytes = !allow ? 0 : allow_stride ? (nq - 1) * allow_stride + nbytes : nbytes;
    const size_t o_pos = 0, o_sc = o_pos + nq * top_k * 4, o_cnt = o_sc + nq * top_k * 4, o_np = o_cnt + nq * 4, o_mm = o_np + nq * 4,
                 o_allow = o_mm + nq * 8, total = o_allow + allow_bytes;
    if ((rc = d.alloc(total))) { (void)hipSetDevice(prev); return rc; }
    Bm25Consumer c;
    c.d_pos = (uint32_t *)(d + o_pos); c.d_scores = (float *)(d + o_sc); c.d_counts = (uint32_t *)(d + o_cnt);
    c.d_npos = (uint32_t *)(d + o_np); c.d_minmax = (float *)(d + o_mm);
    if (allow) {
        if (hipMemcpy(d + o_allow, allow, allow_bytes, hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            leann_set_error("%s: the bitmap could not be copied to the device", fn);
            rc = LEANN_ERR_DEVICE;
        }
        c.d_allow = d + o_allow; c.allow_stride = allow_stride;
    }
    if (rc == LEANN_OK) rc = bm25_run(const_cast<leann_bm25 *>(b), nq, q_off, q_term, q_idf, (uint32_t)top_k, c, nullptr);
    if (rc == LEANN_OK) {
        hipError_t e = hipMemcpy(pos, d + o_pos, nq * top_k * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(scores, d + o_sc, nq * top_k * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(counts, d + o_cnt, nq * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess && n_positive) e = hipMemcpy(n_positive, d + o_np, nq * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess && min_max) e = hipMemcpy(min_max, d + o_mm, nq * 8, hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            leann_set_error("%s: hipMemcpy failed: %s", fn, hipGetErrorString(e));
            rc = LEANN_ERR_DEVICE;
        }
    }
    d.reset(); // before the caller's device is current again
    (void)hipSetDevice(prev);
    return rc;
}

extern "C" int leann_bm25_search_batch(const leann_bm25 *b, size_t nq, const uint32_t *q_off, const uint32_t *q_term, const float *q_idf,
                                       size_t top_k, uint32_t *pos, float *scores, uint32_t *counts, uint32_t *n_positive, float *min_max) {
    return bm25_search_host("leann_bm25_search_batch", b, nq, q_off, q_term, q_idf, top_k, nullptr, 0, pos, scores, counts, n_positive, min_max);
}

extern "C" int leann_bm25_search_filtered_batch(const leann_bm25 *b, size_t nq, const uint32_t *q_off, const uint32_t *q_term, const float *q_idf,
                                                size_t top_k, const uint8_t *allow, size_t allow_stride, uint32_t *pos, float *scores,
                                                uint32_t *counts, uint32_t *n_positive, float *min_max) {
    return bm25_search_host("leann_bm25_search_filtered_batch", b, nq, q_off, q_term, q_idf, top_k, allow, allow_stride, pos, scores, counts,
                            n_positive, min_max);
}

static int bm25_hybrid(const char *fn, const leann_bm25 *b, size_t nq, const uint32_t *q_off, const uint32_t *q_term, const float *q_idf,
                       const uint64_t *d_keys, const float *d_dists, const uint32_t *d_counts, size_t fetch_k, float alpha, int compat_polarity,
                       size_t top_k, const uint8_t *d_allow, size_t allow_stride, uint64_t *d_out_keys, float *d_out_scores,
                       uint32_t *d_out_counts, void *stream) {
    if (fetch_k == 0 || fetch_k > HYB_MAX_FETCH || top_k == 0 || top_k > HYB_MAX_MERGED) {
        leann_set_error("%s: fetch_k %zu outside [1, %d] or top_k %zu outside [1, %d] (the reference fetches 5 * top_k, "
                        "searcher.rs:129-133)", fn, fetch_k, HYB_MAX_FETCH, top_k, HYB_MAX_MERGED);
        return LEANN_ERR_INVALID;
    }
    if (!(alpha >= 0.0f && alpha <= 1.0f)) {
        leann_set_error("%s: alpha %g outside [0, 1]", fn, (double)alpha);
        return LEANN_ERR_INVALID;
    }
    int rc = bm25_check_allow(fn, b, d_allow, allow_stride);
    if (rc == LEANN_OK) rc = bm25_check_search(fn, b, nq, q_off, q_term, q_idf, fetch_k);
    if (rc != LEANN_OK) return rc;
    if (nq == 0) return LEANN_OK;
    if (!d_keys || !d_dists || !d_counts || !d_out_keys || !d_out_scores || !d_out_counts) {
        leann_set_error("%s: null list / output", fn);
        return LEANN_ERR_INVALID;
    }
    Bm25Consumer c;
    c.hybrid = true;
    c.d_keys = d_keys; c.d_dists = d_dists; c.d_vcounts = d_counts;
    c.alpha = alpha; c.compat = compat_polarity; c.top_k = (uint32_t)top_k;
    c.d_out_keys = d_out_keys; c.d_out_scores = d_out_scores; c.d_out_counts = d_out_counts;
    c.d_allow = d_allow; c.allow_stride = allow_stride;
    return bm25_run(const_cast<leann_bm25 *>(b), nq, q_off, q_term, q_idf, (uint32_t)fetch_k, c, (hipStream_t)stream);
}

extern "C" int leann_bm25_hybrid_rerank_device(const leann_bm25 *b, size_t nq, const uint32_t *q_off, const uint32_t *q_term, const float *q_idf,
                                               const uint64_t *d_keys, const float *d_dists, const uint32_t *d_counts, size_t fetch_k, float alpha,
                                               int compat_polarity, size_t top_k, uint64_t *d_out_keys, float *d_out_scores,
                                               uint32_t *d_out_counts, void *stream) {
    return bm25_hybrid("leann_bm25_hybrid_rerank_device", b, nq, q_off, q_term, q_idf, d_keys, d_dists, d_counts, fetch_k, alpha, compat_polarity,
                       top_k, nullptr, 0, d_out_keys, d_out_scores, d_out_counts, stream);
}

extern "C" int leann_bm25_hybrid_rerank_filtered_device(const leann_bm25 *b, size_t nq, const uint32_t *q_off, const uint32_t *q_term,
                                                        const float *q_idf, const uint64_t *d_keys, const float *d_dists,
                                                        const uint32_t *d_counts, size_t fetch_k, float alpha, int compat_polarity, size_t top_k,
                                                        const uint8_t *d_allow, size_t allow_stride, uint64_t *d_out_keys, float *d_out_scores,
                                                        uint32_t *d_out_counts, void *stream) {
    return bm25_hybrid("leann_bm25_hybrid_rerank_filtered_device", b, nq, q_off, q_term, q_idf, d_keys, d_dists, d_counts, fetch_k, alpha,
                       compat_polarity, top_k, d_allow, allow_stride, d_out_keys, d_out_scores, d_out_counts, stream);
}
