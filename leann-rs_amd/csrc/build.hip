// build.hip — on-GPU index construction (needed to HAVE the 1M/10M indexes).
//
// Replaces the arithmetic behind
//     hnsw::build_index / add_to_index   src/backend/hnsw.rs:96-191   (usearch add loop, out of tree)
//     diskann::build_index               src/backend/diskann.rs:70-105 (diskann-rs Vamana, out of tree)
// with batched insertion: points enter in a fixed pseudo-random permutation of their positions (see
// insertion_order below; hnsw.rs:128-130 adds row by row) in batches no larger than the graph built so
// far; every point of a batch
//   1. searches the current graph with the SAME traversal kernel as queries (search.cuh; ef =
//      `complexity`, one launch per level that has new members),
//   2. keeps at most M neighbours by the select-neighbours heuristic (HNSW Alg. 4; Vamana
//      RobustPrune with alpha = 1.2, diskann.rs:91) — a 128x128 candidate Gram matrix per point,
//      LDS-tiled, lower triangle kept in LDS,
//   3. proposes itself to each selected neighbour; proposals are radix-sorted by (target, dist)
//      so that every touched list is rewritten by exactly one workgroup: append while there is
//      room (2M on level 0), otherwise the same heuristic over list ∪ proposals.
// No atomics decide content, so a build is reproducible run to run.  The sequential builders live
// in oracle/oracle.c (orc_hnsw_build / orc_vamana_build); batched insertion is a different schedule,
// so against them graphs are compared by invariants + recall.  The batched schedule itself is restated
// in tests/build_ref.py: on rows with exact f32 dot products a build equals it list for list
// (tests/test_gpu_build_parity.py); inexact rows keep the quality bar.
// An existing graph is continued by continue_build (below): the body of leann_backend_add (a file) and of leann_backend_append[_device]
// (an open handle; tests/test_gpu_append.py, tests/append_ref.py).
#include "common.cuh"
#include "search.cuh"
#include "internal.h"
#include "prune.cuh"
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cstring>
#include <numeric>

#define EXPCAP 256 // expanded nodes recorded per construction search (Vamana)
#define PATHMAX 48 // of which at most this many path nodes join the prune candidates

struct ListView {
    uint32_t *adj0; float *adjd0;  // [n x M0]
    uint32_t *adjU; float *adjdU;  // [n_upper_lists x M]
    const uint32_t *upper_off;
    uint32_t M, M0;
    // Vamana only: per-node PENDING back-edges (ids + distances, [n x P], compact, LEANN_EMPTY padded).  DiskANN lets a list grow to
    // 1.3 R before it re-runs RobustPrune; lists here have a fixed width (R ids), so the slack lives beside the list:
    // a back-edge that finds its target full waits here, invisible to searches, until P of them have gathered; then ONE RobustPrune
    // over list + pending + proposals rewrites the list.  Every touched list being full, the strict rule pruned per proposal:
    // ~600k prunes per 16k-point batch, each gathering 64+ rows (0.4 MB at 1536-d) — 67 % of a 10M x 1536 build.
    uint32_t *pend; float *pendd;
    uint32_t P;
    uint32_t two_stage; // Vamana: occlude_list's two-stage RobustPrune (prune_core)
};
__device__ __forceinline__ void list_ptr(const ListView &lv, uint32_t node, uint32_t level, uint32_t **ids, float **ds,
                                         uint32_t *cap) {
    if (level == 0) {
        *ids = lv.adj0 + (size_t)node * lv.M0;
        *ds = lv.adjd0 + (size_t)node * lv.M0;
        *cap = lv.M0;
    } else {
        size_t o = ((size_t)lv.upper_off[node] + (level - 1)) * lv.M;
        *ids = lv.adjU + o;
        *ds = lv.adjdU + o;
        *cap = lv.M;
    }
}


// ------------------------------------------------------------------------------------------------
// select_kernel: one workgroup per new point of the batch (at one level).
// ------------------------------------------------------------------------------------------------
template <int NC>
__device__ __forceinline__ void select_one(const float *__restrict__ X, uint32_t ld, ListView lv,
                                           const uint32_t *__restrict__ q_rows, uint32_t nq, uint32_t level,
                                           const uint64_t *__restrict__ cand_keys, const float *__restrict__ cand_d,
                                           const uint32_t *__restrict__ cand_cnt, uint32_t efc, uint32_t msel,
                                           float alpha, uint64_t *__restrict__ prop_key, uint32_t *__restrict__ prop_src,
                                           const uint64_t *__restrict__ exp_keys, const uint32_t *__restrict__ exp_cnt,
                                           uint32_t exp_cap) {
    __shared__ __attribute__((aligned(16))) float tri[Pool<NC>::TRI];
    __shared__ uint32_t c_id[NC];
    __shared__ float c_d[NC];
    __shared__ __attribute__((aligned(16))) float wstage[Pool<NC>::STAGE];
    __shared__ uint32_t s_sel[64 * Pool<NC>::KS];
    __shared__ uint32_t s_cnt;
    __shared__ uint64_t pkey[EXPCAP];
    const uint32_t qi = blockIdx.x;
    if (qi >= nq) return;
    const uint32_t q = q_rows[qi];
    uint32_t nc = min(min(cand_cnt[qi], efc), (uint32_t)NC);
    for (uint32_t i = threadIdx.x; i < NC; i += 256) {
        c_id[i] = i < nc ? (uint32_t)cand_keys[(size_t)qi * efc + i] : 0u;
        c_d[i] = i < nc ? cand_d[(size_t)qi * efc + i] : 0.f;
    }
    if (threadIdx.x == 0) s_cnt = NC;
    __syncthreads();
    // a point that is already linked (second Vamana pass) finds itself: drop it from its own candidates
    for (uint32_t i = threadIdx.x; i < nc; i += 256)
        if (c_id[i] == q) s_cnt = i;
    __syncthreads();
    if (s_cnt < nc) {
        const uint32_t self = s_cnt;
        uint32_t mv_id[NC / 256 + 1];
        float mv_d[NC / 256 + 1];
        int t = 0;
        for (uint32_t i = self + threadIdx.x; i + 1 < nc; i += 256, t++) { mv_id[t] = c_id[i + 1]; mv_d[t] = c_d[i + 1]; }
        __syncthreads();
        t = 0;
        for (uint32_t i = self + threadIdx.x; i + 1 < nc; i += 256, t++) { c_id[i] = mv_id[t]; c_d[i] = mv_d[t]; }
        nc--;
        __syncthreads();
    }
    if (exp_keys && nc > 0) {
        // Vamana: prune over the visited set V = final beam  ∪  nodes expanded on the way from the medoid
        // (DiskANN Alg. 2/3).  Path nodes are the expanded entries farther than the beam's worst entry; they
        // supply the long-range edges that keep a single-level graph navigable.
        const uint64_t wmax = ((uint64_t)f32_orderable(c_d[nc - 1]) << 32) | c_id[nc - 1];
        const uint32_t np = min(exp_cnt[qi], min(exp_cap, (uint32_t)EXPCAP));
        for (uint32_t i = threadIdx.x; i < EXPCAP; i += 256) {
            uint64_t key = i < np ? exp_keys[(size_t)qi * exp_cap + i] : ~0ull;
            pkey[i] = (key != ~0ull && key > wmax) ? key : ~0ull;
        }
        for (int size = 2; size <= EXPCAP; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                __syncthreads();
                if (threadIdx.x < EXPCAP / 2) {
                    int i = threadIdx.x;
                    int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                    bool up = ((lo & size) == 0);
                    uint64_t a = pkey[lo], b2 = pkey[hi];
                    if ((a > b2) == up) { pkey[lo] = b2; pkey[hi] = a; }
                }
            }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t n_path = 0;
            while (n_path < EXPCAP && pkey[n_path] != ~0ull) n_path++;
            s_cnt = n_path;
        }
        __syncthreads();
        const uint32_t n_path = s_cnt;
        const uint32_t take = min(n_path, (uint32_t)PATHMAX);
        const uint32_t keep = min(nc, (uint32_t)NC - take);
        __syncthreads();
        for (uint32_t t = threadIdx.x; t < take; t += 256) { // even subsample keeps near and far path nodes
            const uint64_t key = pkey[(uint64_t)t * n_path / take];
            c_id[keep + t] = (uint32_t)key;
            c_d[keep + t] = orderable_f32((uint32_t)(key >> 32));
        }
        nc = keep + take;
        __syncthreads();
    }
    uint32_t ns = prune_core<NC>(X, ld, c_id, c_d, nc, msel, alpha, tri, s_sel, &s_cnt, lv.two_stage != 0, wstage);
    uint32_t *ids; float *ds; uint32_t cap;
    list_ptr(lv, q, level, &ids, &ds, &cap);
    for (uint32_t j = threadIdx.x; j < msel; j += 256) {
        uint64_t pk = ~0ull;
        if (j < ns) {
            uint32_t c = s_sel[j];
            ids[j] = c_id[c];
            ds[j] = c_d[c];
            pk = ((uint64_t)c_id[c] << 32) | f32_orderable(c_d[c]);
        }
        prop_key[(size_t)qi * msel + j] = pk; // (target, dist) ; padding sorts to the end
        prop_src[(size_t)qi * msel + j] = q;
    }
    for (uint32_t j = ns + threadIdx.x; j < cap; j += 256) ids[j] = LEANN_EMPTY; // (a re-linked point: nothing of its old list stays behind the new one)
}

__global__ void __launch_bounds__(256) select_kernel(const float *__restrict__ X, uint32_t ld, ListView lv,
                                                     const uint32_t *__restrict__ q_rows, uint32_t nq, uint32_t level,
                                                     const uint64_t *__restrict__ cand_keys, const float *__restrict__ cand_d,
                                                     const uint32_t *__restrict__ cand_cnt, uint32_t efc, uint32_t msel,
                                                     float alpha, uint64_t *__restrict__ prop_key, uint32_t *__restrict__ prop_src,
                                                     const uint64_t *__restrict__ exp_keys, const uint32_t *__restrict__ exp_cnt,
                                                     uint32_t exp_cap) {
    select_one<NCMAX>(X, ld, lv, q_rows, nq, level, cand_keys, cand_d, cand_cnt, efc, msel, alpha, prop_key, prop_src, exp_keys, exp_cnt, exp_cap);
}
__global__ void __launch_bounds__(256) wide_select_kernel(const float *__restrict__ X, uint32_t ld, ListView lv,
                                                          const uint32_t *__restrict__ q_rows, uint32_t nq, uint32_t level,
                                                          const uint64_t *__restrict__ cand_keys, const float *__restrict__ cand_d,
                                                          const uint32_t *__restrict__ cand_cnt, uint32_t efc, uint32_t msel,
                                                          float alpha, uint64_t *__restrict__ prop_key, uint32_t *__restrict__ prop_src,
                                                          const uint64_t *__restrict__ exp_keys, const uint32_t *__restrict__ exp_cnt,
                                                          uint32_t exp_cap) {
    select_one<NCWIDE>(X, ld, lv, q_rows, nq, level, cand_keys, cand_d, cand_cnt, efc, msel, alpha, prop_key, prop_src, exp_keys, exp_cnt, exp_cap);
}

// heads of equal-target runs in the sorted proposal array
__global__ void segment_heads_kernel(const uint64_t *__restrict__ keys, uint32_t num, uint32_t *__restrict__ seg_start,
                                     uint32_t *__restrict__ nseg) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= num) return;
    uint32_t t = (uint32_t)(keys[i] >> 32);
    if (t == LEANN_EMPTY) return;
    if (i == 0 || (uint32_t)(keys[i - 1] >> 32) != t) seg_start[atomicAdd(nseg, 1u)] = i;
}

// ------------------------------------------------------------------------------------------------
// reverse_merge_kernel: one workgroup per touched list (target node at `level`).
// ------------------------------------------------------------------------------------------------
template <int NC>
__device__ __forceinline__ void reverse_merge_one(const float *__restrict__ X, uint32_t ld, ListView lv,
                                                  uint32_t level, const uint64_t *__restrict__ keys,
                                                  const uint32_t *__restrict__ srcs, uint32_t num,
                                                  const uint32_t *__restrict__ seg_start,
                                                  const uint32_t *__restrict__ nseg_p, float alpha, uint32_t flush_nodes) {
    // flush_nodes != 0: final pass over nodes [0, flush_nodes) — fold whatever is still pending into its list (no proposals)
    __shared__ __attribute__((aligned(16))) float tri[Pool<NC>::TRI];
    __shared__ uint64_t skey[NC];
    __shared__ uint32_t c_id[NC];
    __shared__ float c_d[NC];
    __shared__ __attribute__((aligned(16))) float wstage[Pool<NC>::STAGE];
    __shared__ uint32_t s_sel[64 * Pool<NC>::KS];
    __shared__ uint32_t s_cnt, s_k, s_len, s_pl, s_held;
    uint32_t *const have = reinterpret_cast<uint32_t *>(tri); // the ids the target holds: list at [0, cap), pending at [128, 128 + P)
    const uint32_t nseg = flush_nodes ? flush_nodes : *nseg_p;
    const uint32_t P = level == 0 ? lv.P : 0u;
    for (uint32_t seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
        const uint32_t start = flush_nodes ? 0u : seg_start[seg];
        const uint32_t t = flush_nodes ? seg : (uint32_t)(keys[start] >> 32);
        uint32_t *ids; float *ds; uint32_t cap;
        list_ptr(lv, t, level, &ids, &ds, &cap);
        uint32_t *pid = P ? lv.pend + (size_t)t * P : nullptr;
        float *pdd = P ? lv.pendd + (size_t)t * P : nullptr;
        if (threadIdx.x == 0) { s_k = 0; s_len = 0; s_pl = 0; s_held = 0; }
        __syncthreads();
        // proposals of this run (sorted by dist): count up to NC; existing list / pending lengths
        if (!flush_nodes && threadIdx.x < NC) {
            uint32_t i = start + threadIdx.x;
            if (i < num && (uint32_t)(keys[i] >> 32) == t) atomicAdd(&s_k, 1u); // run is contiguous
        }
        if (threadIdx.x < cap) {
            const uint32_t e = ids[threadIdx.x];
            have[threadIdx.x] = e;
            if (e != LEANN_EMPTY) atomicAdd(&s_len, 1u); // lists are compact
        }
        if (threadIdx.x >= 64 && threadIdx.x < 64 + P) {
            const uint32_t e = pid[threadIdx.x - 64];
            have[128 + threadIdx.x - 64] = e;
            if (e != LEANN_EMPTY) atomicAdd(&s_pl, 1u);
        }
        __syncthreads();
        const uint32_t len = s_len, pl = s_pl;
        uint32_t k = s_k;
        if (flush_nodes && pl == 0) { __syncthreads(); continue; }
        if (!flush_nodes) {
            // The run moves into LDS (c_id / c_d, free until the sorted pool is written), without the proposals whose source the list
            // or the pending area holds already: a refine pass (LEANN_VAMANA_PASSES) re-links points that are linked, and a source
            // appended or merged a second time would stand in the list twice.  The order of the others is kept.  k <= NC <= 256:
            // thread j owns proposal j.
            const bool mine = threadIdx.x < k;
            uint32_t src = 0;
            float dj = 0.f;
            bool held = false;
            if (mine) {
                src = srcs[start + threadIdx.x];
                dj = orderable_f32((uint32_t)keys[start + threadIdx.x]);
                for (uint32_t i = 0; i < len; i++) held |= have[i] == src;
                for (uint32_t i = 0; i < pl; i++) held |= have[128 + i] == src;
                if (held) atomicAdd(&s_held, 1u);
            }
            if (threadIdx.x < NC) skey[threadIdx.x] = (mine && !held) ? 1ull : 0ull;
            __syncthreads();
            const uint32_t n_held = s_held;
            if (mine && !held) {
                uint32_t pos = threadIdx.x;
                if (n_held) { // (never in a first pass: its sources are new to the graph)
                    pos = 0;
                    for (uint32_t i = 0; i < threadIdx.x; i++) pos += (uint32_t)skey[i];
                }
                c_id[pos] = src;
                c_d[pos] = dj;
            }
            k -= n_held;
            __syncthreads();
            if (k == 0) continue;
        }
        const uint32_t room = cap - len;
        if (!flush_nodes && k <= room + (P - pl)) {
            // room in the list (visible at once, closest proposals first), then in the pending area: plain appends in (dist, src) order
            for (uint32_t j = threadIdx.x; j < k; j += 256) {
                const uint32_t src = c_id[j];
                const float dj = c_d[j];
                if (j < room) { ids[len + j] = src; ds[len + j] = dj; }
                else { pid[pl + j - room] = src; pdd[pl + j - room] = dj; }
            }
            __syncthreads();
            continue;
        }
        if (len + pl + k > NC) k = NC - len - pl; // keep the closest proposals only
        const uint32_t nc = len + pl + k;
        for (uint32_t i = threadIdx.x; i < NC; i += 256) {
            uint64_t key = ~0ull;
            if (i < len) key = ((uint64_t)f32_orderable(ds[i]) << 32) | ids[i];
            else if (i < len + pl) key = ((uint64_t)f32_orderable(pdd[i - len]) << 32) | pid[i - len];
            else if (i < nc) key = ((uint64_t)f32_orderable(c_d[i - len - pl]) << 32) | c_id[i - len - pl];
            skey[i] = key;
        }
        // bitonic sort of NC keys by (dist, id)
        for (int size = 2; size <= NC; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                __syncthreads();
                if (threadIdx.x < NC / 2) {
                    int i = threadIdx.x;
                    int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                    bool up = ((lo & size) == 0);
                    uint64_t a = skey[lo], b = skey[hi];
                    if ((a > b) == up) { skey[lo] = b; skey[hi] = a; }
                }
            }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < NC; i += 256) {
            c_id[i] = i < nc ? (uint32_t)skey[i] : 0u;
            c_d[i] = i < nc ? orderable_f32((uint32_t)(skey[i] >> 32)) : 0.f;
        }
        __syncthreads();
        uint32_t ns = prune_core<NC>(X, ld, c_id, c_d, nc, cap, alpha, tri, s_sel, &s_cnt, lv.two_stage != 0, wstage);
        for (uint32_t j = threadIdx.x; j < cap; j += 256) {
            if (j < ns) {
                uint32_t c = s_sel[j];
                ids[j] = c_id[c];
                ds[j] = c_d[c];
            } else {
                ids[j] = LEANN_EMPTY;
                ds[j] = 0.f;
            }
        }
        for (uint32_t j = threadIdx.x; j < P; j += 256) { pid[j] = LEANN_EMPTY; pdd[j] = 0.f; }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) reverse_merge_kernel(const float *__restrict__ X, uint32_t ld, ListView lv,
                                                            uint32_t level, const uint64_t *__restrict__ keys,
                                                            const uint32_t *__restrict__ srcs, uint32_t num,
                                                            const uint32_t *__restrict__ seg_start,
                                                            const uint32_t *__restrict__ nseg_p, float alpha, uint32_t flush_nodes) {
    reverse_merge_one<NCMAX>(X, ld, lv, level, keys, srcs, num, seg_start, nseg_p, alpha, flush_nodes);
}
__global__ void __launch_bounds__(256) wide_reverse_merge_kernel(const float *__restrict__ X, uint32_t ld, ListView lv,
                                                                 uint32_t level, const uint64_t *__restrict__ keys,
                                                                 const uint32_t *__restrict__ srcs, uint32_t num,
                                                                 const uint32_t *__restrict__ seg_start,
                                                                 const uint32_t *__restrict__ nseg_p, float alpha, uint32_t flush_nodes) {
    reverse_merge_one<NCWIDE>(X, ld, lv, level, keys, srcs, num, seg_start, nseg_p, alpha, flush_nodes);
}

__global__ void fill_u32_kernel(uint32_t *p, size_t n, uint32_t v) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}
__global__ void col_partial_kernel(const float *__restrict__ X, size_t n, uint32_t d, uint32_t ld, uint32_t S,
                                   double *__restrict__ part /* [S x ld] */) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x, sl = blockIdx.y;
    if (j >= ld) return;
    double s = 0.0;
    if (j < d)
        for (size_t i = sl; i < n; i += S) s += X[i * ld + j];
    part[(size_t)sl * ld + j] = s;
}
__global__ void col_mean_kernel(const double *__restrict__ part, size_t n, uint32_t ld, uint32_t S, float *__restrict__ mean) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ld) return;
    double s = 0.0;
    for (uint32_t sl = 0; sl < S; sl++) s += part[(size_t)sl * ld + j];
    mean[j] = (float)(s / (double)n);
}

// Stored link distances of an existing graph (the index file does not carry them): one wave per node walks its level-0
// list and its upper lists and recomputes dist(node, neighbour) with the canonical wave dot — bit-identical to the value
// the construction search produced when the link was made (fmaf is symmetric in its factors), so an append continues
// exactly from the state a one-shot build would have had.
__global__ void __launch_bounds__(256) link_dist_kernel(const float *__restrict__ X, uint32_t ld, ListView lv,
                                                        const uint8_t *__restrict__ levels, uint32_t n_nodes) {
    const uint32_t node = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (node >= n_nodes) return;
    const float *xi = X + (size_t)node * ld;
    const int T = (int)((ld + 255) / 256);
    const uint32_t top = levels[node];
    for (uint32_t level = 0; level <= top; level++) {
        uint32_t *ids; float *ds; uint32_t cap;
        list_ptr(lv, node, level, &ids, &ds, &cap);
        for (uint32_t j = 0; j < cap; j++) {
            const uint32_t e = ids[j];
            if (e == LEANN_EMPTY) break; // lists are compact
            const float *xe = X + (size_t)e * ld;
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int t = 0; t < T; t++) fma4(acc, row_load4(xi, ld, t, lane), row_load4(xe, ld, t, lane));
            const float d = 1.0f - wave_tree_sum(lane4_sum(acc));
            if (lane == 0) ds[j] = d;
        }
    }
}

// ------------------------------------------------------------------------------------------------
struct Builder {
    leann_backend *h;
    ListView lv{};
    DeviceBuf<float> adjd0, adjdU;
    DeviceBuf<uint32_t> pend; DeviceBuf<float> pendd; // Vamana: pending back-edges (ListView)
    std::vector<uint8_t> levels;     // host copy
    std::vector<uint32_t> upper_off; // host copy
    DeviceBuf<uint32_t> d_order;     // insertion order (device copy)
    std::vector<uint32_t> order;     // ... host copy: order[j] = position inserted j-th
    std::vector<uint32_t> h_order_first; // only used for Vamana (medoid first)
    // per-batch scratch
    size_t bmax = 0;
    DeviceBuf<uint64_t> cand_keys, candU_keys, prop_key, prop_key2, exp_keys; // (exp_*: Vamana only)
    DeviceBuf<float> cand_d, candU_d;
    DeviceBuf<uint32_t> cand_cnt, candU_cnt, d_rowsU, prop_src, prop_src2, seg_start, nseg, exp_cnt;
    DeviceBuf<unsigned char> cub_tmp; size_t cub_bytes = 0;
    hipStream_t st = nullptr;
    size_t batch_fraction = 8; // LEANN_BUILD_BATCH_FRACTION, read once per build
    float alpha_now = 1.2f;    // Vamana: RobustPrune's alpha of the pass under way
    Builder() = default;
    Builder(const Builder &) = delete;
    ~Builder() { // every exit of build_on_device, including the error returns, releases the scratch and the stream
        if (st) (void)hipStreamSynchronize(st); // in the body: the members are freed after it, when no kernel of the build still runs
        if (st) (void)hipStreamDestroy(st);
    }
};
// construction knobs are read once per build (a build takes seconds to minutes; the search path reads no environment at all)
static int env_int(const char *name, int dflt, int lo, int hi) {
    const char *e = getenv(name);
    if (!e || !*e) return dflt;
    const int v = atoi(e);
    return v >= lo && v <= hi ? v : dflt;
}

#define BCHECK(expr)                                                                           \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) {                                                                \
            leann_set_error("build: %s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return LEANN_ERR_DEVICE;                                                           \
        }                                                                                      \
    } while (0)

static int link_level(Builder &b, const uint32_t *d_rows, uint32_t nq, uint32_t level, const uint64_t *ck, const float *cd,
                      const uint32_t *cc, const uint64_t *ek = nullptr, const uint32_t *ec = nullptr) {
    leann_backend *h = b.h;
    const uint32_t efc = h->efc, msel = h->g.M; // M new links per point on every level (Malkov Alg. 1)
    const float alpha = h->kind == LEANN_BACKEND_DISKANN ? b.alpha_now : 0.f;
    const bool wide = std::max(h->g.M0, h->g.M) > 64; // lists of up to 128 ids: 256-candidate pools (NCWIDE)
    hipLaunchKernelGGL(wide ? wide_select_kernel : select_kernel, dim3(nq), dim3(256), 0, b.st, h->g.X, h->g.ld, b.lv, d_rows, nq, level,
                       ck, cd, cc, efc, msel, alpha, b.prop_key, b.prop_src, ek, ec, (uint32_t)EXPCAP);
    const uint32_t num = nq * msel;
    size_t tmp = b.cub_bytes;
    BCHECK(hipcub::DeviceRadixSort::SortPairs(b.cub_tmp.p, tmp, b.prop_key.p, b.prop_key2.p, b.prop_src.p, b.prop_src2.p, (int)num, 0, 64, b.st));
    BCHECK(hipMemsetAsync(b.nseg, 0, 4, b.st));
    hipLaunchKernelGGL(segment_heads_kernel, dim3((num + 255) / 256), dim3(256), 0, b.st, b.prop_key2, num, b.seg_start, b.nseg);
    uint32_t grid = std::min<uint32_t>(num, 256 * 16);
    hipLaunchKernelGGL(wide ? wide_reverse_merge_kernel : reverse_merge_kernel, dim3(grid), dim3(256), 0, b.st, h->g.X, h->g.ld, b.lv,
                       level, b.prop_key2, b.prop_src2, num, b.seg_start, b.nseg, alpha, 0u);
    BCHECK(hipGetLastError());
    return LEANN_OK;
}

static int builder_alloc_scratch(Builder &b, size_t bmax) {
    leann_backend *h = b.h;
    const size_t efc = h->efc, msel = h->g.M;
    b.bmax = bmax;
    const size_t bu = bmax / 16 + 64; // upper-level members per batch (expected bmax/31)
    if (b.cand_keys.alloc(bmax * efc) || b.cand_d.alloc(bmax * efc) || b.cand_cnt.alloc(bmax) || b.candU_keys.alloc(bu * efc * 16) ||
        b.candU_d.alloc(bu * efc * 16) || b.candU_cnt.alloc(bu * 16) || b.d_rowsU.alloc(bu * 16) || b.prop_key.alloc(bmax * msel) ||
        b.prop_key2.alloc(bmax * msel) || b.prop_src.alloc(bmax * msel) || b.prop_src2.alloc(bmax * msel) ||
        b.seg_start.alloc(bmax * msel) || b.nseg.alloc(4))
        return LEANN_ERR_DEVICE;
    if (h->kind == LEANN_BACKEND_DISKANN && (b.exp_keys.alloc(bmax * EXPCAP) || b.exp_cnt.alloc(bmax))) return LEANN_ERR_DEVICE;
    size_t tmp = 0;
    BCHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, b.prop_key.p, b.prop_key2.p, b.prop_src.p, b.prop_src2.p,
                                              (int)(bmax * msel), 0, 64, b.st));
    b.cub_bytes = tmp;
    return b.cub_tmp.alloc(tmp);
}

// Insert order[s0 .. n) into the graph that already holds order[0 .. s0).
static int builder_insert_range(Builder &b, const std::vector<uint32_t> &order_host_upper /* unused */, size_t s0, size_t n,
                                bool refine = false) {
    (void)order_host_upper;
    leann_backend *h = b.h;
    const uint32_t efc = h->efc;
    const bool hnsw = h->kind == LEANN_BACKEND_HNSW || h->nav_levels; // (leveled: entry layers above the base graph)
    size_t s = s0;
    const size_t bu_cap = (b.bmax / 16 + 64) * 16;
    while (s < n) {
        // A batch's points do not see each other, so a batch must stay a small fraction of the graph it is inserted into: at most
        // 1/8 (LEANN_BUILD_BATCH_FRACTION) of the points already linked.  With batches as large as the graph itself — the first
        // rule here — two thirds of a 50k-row index went in without seeing their batch mates and recall@10 at ef = 32 fell 1.6
        // points below the sequential builder's (tests/test_gpu_builder_quality.py); from ~130k rows on the cap is bmax anyway.
        const size_t frac = b.batch_fraction;
        size_t B = std::min<size_t>(std::min<size_t>(b.bmax, refine ? b.bmax : std::max<size_t>(1, s / frac)), n - s);
        const uint32_t Lmax = h->g.max_level;
        // ---- phase 1: searches (graph does not contain any point of the batch yet) ----------------
        struct LevelJob { uint32_t level, nq; size_t off; };
        std::vector<LevelJob> jobs;
        size_t offU = 0;
        if (hnsw && Lmax > 0) {
            for (uint32_t l = Lmax; l >= 1; --l) {
                std::vector<uint32_t> rows;
                for (size_t i = s; i < s + B; i++)
                    if (b.levels[b.order[i]] >= l) rows.push_back(b.order[i]);
                if (rows.empty()) continue;
                if (offU + rows.size() > bu_cap) {
                    leann_set_error("build: upper-level scratch exhausted");
                    return LEANN_ERR_DEVICE;
                }
                BCHECK(hipMemcpyAsync(b.d_rowsU + offU, rows.data(), rows.size() * 4, hipMemcpyHostToDevice, b.st));
                BCHECK(hipStreamSynchronize(b.st)); // rows is a stack temporary
                SearchArgs a{};
                a.q_rows = b.d_rowsU + offU;
                a.nq = (uint32_t)rows.size();
                a.k = efc;
                a.ef = efc;
                a.target_level = l;
                a.out_keys = b.candU_keys + offU * efc;
                a.out_dists = b.candU_d + offU * efc;
                a.out_counts = b.candU_cnt + offU;
                int rc = leann_internal_launch_search(h, a, b.st);
                if (rc) return rc;
                jobs.push_back({l, (uint32_t)rows.size(), offU});
                offU += rows.size();
            }
        }
        {
            SearchArgs a{};
            a.q_rows = b.d_order + s;
            a.nq = (uint32_t)B;
            a.k = efc;
            a.ef = efc;
            a.target_level = 0;
            a.out_keys = b.cand_keys;
            a.out_dists = b.cand_d;
            a.out_counts = b.cand_cnt;
            a.out_expanded = b.exp_keys; // null for HNSW
            a.out_nexp = b.exp_cnt;
            a.exp_cap = EXPCAP;
            int rc = leann_internal_launch_search(h, a, b.st);
            if (rc) return rc;
        }
        // ---- phase 2: select + link, level by level ---------------------------------------------
        for (auto &j : jobs) {
            int rc = link_level(b, b.d_rowsU + j.off, j.nq, j.level, b.candU_keys + j.off * efc, b.candU_d + j.off * efc,
                                b.candU_cnt + j.off);
            if (rc) return rc;
        }
        int rc = link_level(b, b.d_order + s, (uint32_t)B, 0, b.cand_keys, b.cand_d, b.cand_cnt, b.exp_keys, b.exp_cnt);
        if (rc) return rc;
        // ---- entry point / top level (sequential semantics of hnsw.rs:128-130 within the batch) --
        if (hnsw)
            for (size_t i = s; i < s + B; i++)
                if (b.levels[b.order[i]] > h->g.max_level) { h->g.max_level = b.levels[b.order[i]]; h->g.entry = b.order[i]; }
        s += B;
    }
    BCHECK(hipStreamSynchronize(b.st));
    return LEANN_OK;
}

// Insertion order.  A batch is inserted against the graph of the batches before it (its points do not see each other), so every
// batch must be a representative sample of the rows still to come: inserting in storage order breaks on data stored topic by topic
// (a 10M-row corpus laid out cluster-major and built in id order: recall@10 0.20 at ef = 56, against 0.957 for the same rows stored
// in hashed order).  The rows [lo, n) are therefore inserted in a fixed pseudo-random permutation (positions sorted by a hash of
// the position): 0.957 for both layouts.  (A golden-ratio stride permutation was tried first: fine on the cluster-major layout,
// 0.947 on the hashed one.)  Rows [0, lo) (an existing index) keep their places.  `pin_first`: that position is inserted first
// (Vamana medoid).  Returns order[lo].
static uint32_t insertion_order(std::vector<uint32_t> &order, size_t lo, size_t n, const uint32_t *pin_first = nullptr) {
    order.resize(std::max<size_t>(n, 1));
    for (size_t i = 0; i < lo; i++) order[i] = (uint32_t)i;
    const uint64_t m = n - lo;
    if (m == 0) return 0;
    size_t w = lo;
    if (pin_first) order[w++] = *pin_first;
    // pseudo-random permutation: positions sorted by a hash of the position (ties impossible: the position is part of the key)
    std::vector<uint64_t> keyed(m);
    for (uint64_t j = 0; j < m; j++) keyed[j] = (mix64((lo + j) ^ 0x4F52444552ull) & 0xFFFFFFFF00000000ull) | (uint32_t)(lo + j);
    std::sort(keyed.begin(), keyed.end());
    for (uint64_t j = 0; j < m; j++) {
        const uint32_t pos = (uint32_t)keyed[j];
        if (pin_first && pos == *pin_first) continue;
        order[w++] = pos;
    }
    return order[lo];
}

static int build_on_device(leann_backend *h, size_t n_existing, size_t bmax_hint, bool keep_prune_form = false) {
    // h->g.X / n / d / ld / M / M0 / kind / efc / alpha are set; adjacency arrays allocated & initialised
    // for nodes < n_existing (append) or empty.  keep_prune_form: Vamana prunes by h->two_stage as it stands (the form the graph
    // being continued was built with), not by LEANN_VAMANA_TWO_STAGE.
    Builder b;
    b.h = h;
    b.batch_fraction = (size_t)env_int("LEANN_BUILD_BATCH_FRACTION", 8, 1, 1 << 20);
    const size_t n = h->g.n;
    BCHECK(hipStreamCreateWithFlags(&b.st, hipStreamNonBlocking));
    b.lv.adj0 = h->store.adj0;
    b.lv.adjU = h->store.adjU;
    b.lv.upper_off = h->g.upper_off;
    b.lv.M = h->g.M;
    b.lv.M0 = h->g.M0;
    const size_t nu = std::max<size_t>(h->n_upper_lists, 1);
    if (b.adjd0.alloc(std::max<size_t>(n, 1) * h->g.M0) || b.adjdU.alloc(nu * h->g.M)) return LEANN_ERR_DEVICE;
    BCHECK(hipMemset(b.adjd0, 0, std::max<size_t>(n, 1) * h->g.M0 * 4));
    BCHECK(hipMemset(b.adjdU, 0, nu * h->g.M * 4));
    b.lv.adjd0 = b.adjd0;
    b.lv.adjdU = b.adjdU;
    if (h->kind == LEANN_BACKEND_DISKANN) { // slack of DiskANN's 1.3 R, kept beside the 64-slot lists (see ListView)
        // 10M x 1536, R = 64, recall@10 at L = 72 over 2 000 queries (scripts/exp/vamana_slack.sh): strict (0 pending) 185.8 s / 0.9600;
        // 4 pending 82.2 s / 0.9596; 8: 65.3 s / 0.9531; 16: 56.1 s / 0.9547.  Back-edges that wait are invisible to the construction
        // searches of later points, which costs about half a point of recall from 8 on; 4 keeps the strict rule's recall at 2.3x its speed.
        b.lv.two_stage = keep_prune_form ? h->two_stage : (uint32_t)env_int("LEANN_VAMANA_TWO_STAGE", 1, 0, 1);
        h->two_stage = b.lv.two_stage; // delete consolidation repairs with the rule the build used
        const uint32_t slack = (uint32_t)env_int("LEANN_VAMANA_PENDING", 4, 0, 32);
        b.lv.P = slack;
        if (slack) {
            if (b.pend.alloc(std::max<size_t>(n, 1) * slack) || b.pendd.alloc(std::max<size_t>(n, 1) * slack)) return LEANN_ERR_DEVICE;
            BCHECK(hipMemset(b.pend, 0xFF, std::max<size_t>(n, 1) * slack * 4));
            BCHECK(hipMemset(b.pendd, 0, std::max<size_t>(n, 1) * slack * 4));
            b.lv.pend = b.pend;
            b.lv.pendd = b.pendd;
        }
    }
    b.levels.resize(std::max<size_t>(n, 1));
    BCHECK(hipMemcpy(b.levels.data(), h->store.levels, n, hipMemcpyDeviceToHost));
    if (int rc = b.d_order.alloc(std::max<size_t>(n, 1))) return rc;
    int rc = LEANN_OK;
    size_t s0 = n_existing;
    if (n_existing == 0 && n > 0) {
        uint32_t first = 0;
        if (h->kind == LEANN_BACKEND_DISKANN && !h->nav_levels) {
            // medoid: closest row to the mean direction, by the index metric (ties -> lower id)
            DeviceBuf<float> mean, ms;
            DeviceBuf<uint64_t> mk;
            DeviceBuf<uint32_t> mc;
            DeviceBuf<double> part;
            const uint32_t S = 1024;
            if (mean.alloc(h->g.ld) || mk.alloc(1) || ms.alloc(1) || mc.alloc(1) || part.alloc((size_t)S * h->g.ld)) return LEANN_ERR_DEVICE;
            hipLaunchKernelGGL(col_partial_kernel, dim3((h->g.ld + 63) / 64, S), dim3(64), 0, b.st, h->g.X, n, h->g.d, h->g.ld, S, part);
            hipLaunchKernelGGL(col_mean_kernel, dim3((h->g.ld + 63) / 64), dim3(64), 0, b.st, part, n, h->g.ld, S, mean);
            BCHECK(hipStreamSynchronize(b.st));
            rc = leann_scan_topk_device(h->g.X, n, h->g.d, h->g.ld, mean, 1, 1, nullptr, 0, mk, ms, mc, b.st);
            if (rc) return rc;
            uint64_t key = 0;
            BCHECK(hipMemcpyAsync(&key, mk, 8, hipMemcpyDeviceToHost, b.st));
            BCHECK(hipStreamSynchronize(b.st));
            first = (uint32_t)key;
        }
        const bool leveled = h->kind == LEANN_BACKEND_HNSW || h->nav_levels;
        if (leveled) first = insertion_order(b.order, 0, n);
        else insertion_order(b.order, 0, n, &first);
        h->g.entry = first;
        h->g.max_level = leveled ? b.levels[first] : 0;
        s0 = 1;
    } else {
        insertion_order(b.order, n_existing, n);
        // append: the existing links' stored distances (read by reverse_merge_kernel when a list is pruned)
        hipLaunchKernelGGL(link_dist_kernel, dim3((unsigned)((n_existing + 3) / 4)), dim3(256), 0, b.st, h->g.X, h->g.ld, b.lv, h->store.levels.p,
                           (uint32_t)n_existing);
        BCHECK(hipGetLastError());
    }
    BCHECK(hipMemcpyAsync(b.d_order, b.order.data(), n * 4, hipMemcpyHostToDevice, b.st));
    size_t bmax = bmax_hint ? bmax_hint : 16384;
    rc = builder_alloc_scratch(b, bmax);
    const int passes = env_int("LEANN_VAMANA_PASSES", 1, 1, 3);
    b.alpha_now = h->alpha;
    if (passes > 1 && h->kind == LEANN_BACKEND_DISKANN) { // experiment knob: alpha of every pass but the last (DiskANN: 1.0), in 1/100
        b.alpha_now = (float)env_int("LEANN_VAMANA_ALPHA1_PCT", (int)(h->alpha * 100.f + 0.5f), 100, 400) / 100.f;
    }
    if (rc == LEANN_OK) rc = builder_insert_range(b, {}, s0, n);
    // DiskANN builds in two passes over the points (the second one re-links every point against the finished graph).  Optional here
    // (LEANN_VAMANA_PASSES=2), off by default — 10M x 1536: at R = 64 it doubles the build (82 -> 173 s) and buys nothing (recall@10 0.95
    // needs L = 76 instead of 72); at R = 32, where one pass is not enough for 10M clustered rows (recall 0.60 at L = 128), it lifts the
    // recall to 0.81 — still not a usable index, which is why the 10M benchmarks use R = 64.
    for (int p = 1; rc == LEANN_OK && p < passes && h->kind == LEANN_BACKEND_DISKANN && n_existing == 0 && n > 1; p++) {
        if (p == passes - 1) b.alpha_now = h->alpha;
        rc = builder_insert_range(b, {}, 0, n, true);
    }
    b.alpha_now = h->alpha;
    if (rc == LEANN_OK && b.lv.P && n) { // fold what is still pending into the lists (DiskANN's final trim)
        const float alpha = h->alpha;
        hipLaunchKernelGGL(std::max(h->g.M0, h->g.M) > 64 ? wide_reverse_merge_kernel : reverse_merge_kernel, dim3(256 * 16), dim3(256), 0,
                           b.st, h->g.X, h->g.ld, b.lv, 0u, (const uint64_t *)nullptr,
                           (const uint32_t *)nullptr, 0u, (const uint32_t *)nullptr, (const uint32_t *)nullptr, alpha, (uint32_t)n);
        BCHECK(hipGetLastError());
        BCHECK(hipStreamSynchronize(b.st));
    }
    return rc; // ~Builder: stream synchronised, scratch freed
}

// levels / upper_off on host (orc_level twin: common.cuh:node_level), uploaded once
// `levels`: at least max(n, 1) entries; positions from `hash_from` on get the builder's hash of the position (what is in front of
// them is the caller's: the levels of an existing graph), upper_off is the exclusive prefix sum of the whole table
static int alloc_graph_arrays(leann_backend *h, uint64_t level_seed, std::vector<uint8_t> &levels, size_t hash_from) {
    const size_t n = h->g.n, nn = std::max<size_t>(n, 1);
    if (h->kind == LEANN_BACKEND_HNSW || h->nav_levels)
        for (size_t i = hash_from; i < n; i++) levels[i] = (uint8_t)node_level(level_seed, i, h->g.M);
    std::vector<uint32_t> uo(nn, 0);
    if (int rc = leann_internal_alloc_graph_lists(h, leann_internal_upper_offsets(levels.data(), n, uo.data()))) return rc;
    BCHECK(hipMemset(h->store.adj0, 0xFF, nn * h->g.M0 * 4)); // the builder's lists start empty
    BCHECK(hipMemcpy(h->store.upper_off, uo.data(), nn * 4, hipMemcpyHostToDevice));
    BCHECK(hipMemcpy(h->store.levels, levels.data(), nn, hipMemcpyHostToDevice));
    return LEANN_OK;
}
static int alloc_graph_arrays(leann_backend *h, uint64_t level_seed) { // a fresh build: every level is the hash
    std::vector<uint8_t> levels(std::max<size_t>(h->g.n, 1), 0);
    return alloc_graph_arrays(h, level_seed, levels, 0);
}

static constexpr uint64_t LEVEL_SEED = 0x5EED0003ull;

static int build_device_impl(int backend, const float *d_vectors, size_t n, size_t dims, size_t ld, size_t graph_degree, size_t complexity,
                             int device, uint64_t key_offset, int take_copy, leann_backend **out, bool planes);
// The backend, and its list lengths: lists hold at most 128 ids, HNSW graph_degree M in [2, 64] (level 0 keeps 2 M), DiskANN R in
// [2, 128].  Every build entry point checks them here, before any device work.
int leann_internal_check_build_args(int backend, size_t graph_degree, size_t complexity) {
    if (backend != LEANN_BACKEND_HNSW && backend != LEANN_BACKEND_DISKANN) {
        leann_set_error("Unknown backend: %d", backend);
        return LEANN_ERR_INVALID;
    }
    const size_t maxdeg = backend == LEANN_BACKEND_HNSW ? 64 : 128;
    if (graph_degree < 2 || graph_degree > maxdeg || complexity < 1) {
        leann_set_error("build: graph_degree must be in [2, %zu] (%s) and complexity >= 1 (got %zu, %zu)", maxdeg,
                        backend == LEANN_BACKEND_HNSW ? "hnsw" : "diskann", graph_degree, complexity);
        return LEANN_ERR_INVALID;
    }
    return LEANN_OK;
}
// `planes`: cut the row screen's split planes (planes.hip) for the new handle — not for one that is only saved and closed again
static int build_device_guarded(int backend, const float *d_vectors, size_t n, size_t dims, size_t ld, size_t graph_degree, size_t complexity,
                                int device, uint64_t key_offset, int take_copy, leann_backend **out, bool planes) {
    try { // host-side bookkeeping of the builder allocates (insertion order, level tables): nothing may be thrown across the C ABI
        return build_device_impl(backend, d_vectors, n, dims, ld, graph_degree, complexity, device, key_offset, take_copy, out, planes);
    } catch (const std::exception &e) {
        leann_set_error("build: %s", e.what());
        return LEANN_ERR_DEVICE;
    }
}
extern "C" int leann_backend_build_device(int backend, const float *d_vectors, size_t n, size_t dims, size_t ld,
                                          size_t graph_degree, size_t complexity, int device, uint64_t key_offset,
                                          int take_copy, leann_backend **out) {
    return build_device_guarded(backend, d_vectors, n, dims, ld, graph_degree, complexity, device, key_offset, take_copy, out, true);
}
// the device build WITHOUT the row screen's split planes: for a caller that replaces the f32 rows afterwards (narrow_rows.hip) — the
// planes would be a second full-size copy of rows that are about to go
int leann_internal_build_device_no_planes(int backend, const float *d_vectors, size_t n, size_t dims, size_t ld, size_t graph_degree,
                                          size_t complexity, int device, uint64_t key_offset, leann_backend **out) {
    return build_device_guarded(backend, d_vectors, n, dims, ld, graph_degree, complexity, device, key_offset, 0, out, false);
}
static int build_device_impl(int backend, const float *d_vectors, size_t n, size_t dims, size_t ld, size_t graph_degree, size_t complexity,
                             int device, uint64_t key_offset, int take_copy, leann_backend **out, bool planes) {
    if (!out || (n && !d_vectors) || dims == 0 || dims > 4096 || ld < dims || (ld & 3) || n >= (1ull << 31)) {
        leann_set_error("leann_backend_build_device: invalid arguments (n=%zu dims=%zu ld=%zu)", n, dims, ld);
        return LEANN_ERR_INVALID;
    }
    if (int rc = leann_internal_check_build_args(backend, graph_degree, complexity)) return rc;
    if (int rc = leann_internal_check_device(device)) return rc;
    BCHECK(hipSetDevice(device));
    leann_backend *h = new leann_backend();
    h->kind = backend;
    h->device = device;
    h->key_offset = key_offset;
    h->efc = (uint32_t)std::max<size_t>(complexity, graph_degree);
    h->alpha = 1.2f; // diskann.rs:91
    h->g.n = n;
    h->g.d = (uint32_t)dims;
    h->g.ld = (uint32_t)ld;
    h->g.M = (uint32_t)graph_degree;
    h->g.M0 = backend == LEANN_BACKEND_HNSW ? (uint32_t)(2 * graph_degree) : (uint32_t)graph_degree;
    h->nav_levels = backend == LEANN_BACKEND_DISKANN && env_int("LEANN_VAMANA_NAV", 0, 0, 1) != 0;
    if (take_copy) {
        DeviceBuf<float> cp;
        if (cp.alloc(std::max<size_t>(n * ld, 4)) || (n && hipMemcpy(cp, d_vectors, n * ld * 4, hipMemcpyDeviceToDevice) != hipSuccess)) {
            leann_set_error("build: copying %zu rows failed: %s", n, hipGetErrorString(hipGetLastError()));
            leann_backend_close(h);
            return LEANN_ERR_DEVICE;
        }
        leann_internal_own_rows(h, std::move(cp));
    } else {
        h->g.X = d_vectors; // borrowed: store.rows stays empty
    }
    int rc = alloc_graph_arrays(h, LEVEL_SEED);
    if (rc == LEANN_OK && n) rc = build_on_device(h, 0, 0);
    if (rc) { leann_backend_close(h); return rc; }
    if (planes) leann_internal_sync_planes(h);
    *out = h;
    return LEANN_OK;
}

// BackendBuilder::build — src/backend/mod.rs:55-79
extern "C" int leann_backend_build(int backend, const float *vectors, size_t n, size_t dims, size_t graph_degree,
                                   size_t complexity, const char *index_path_stem) {
    if (!index_path_stem || (n && !vectors) || dims == 0) {
        leann_set_error("leann_backend_build: invalid arguments");
        return LEANN_ERR_INVALID;
    }
    if (int rc = leann_internal_check_build_args(backend, graph_degree, complexity)) return rc;
    if (int rc = leann_internal_use_device0()) return rc;
    const size_t ld = (dims + 3) & ~(size_t)3;
    DeviceBuf<float> dX; // this call's own copy: the handle below borrows it and is closed before it goes
    if (int rc = dX.alloc(std::max<size_t>(n * ld, 4))) return rc;
    BCHECK(leann_internal_stage_rows(dX, ld, vectors, dims, dims, n, true));
    leann_backend *h = nullptr;
    int rc = build_device_guarded(backend, dX, n, dims, ld, graph_degree, complexity, 0, 0, 0, &h, false);
    if (rc) return rc;
    rc = leann_backend_save(h, index_path_stem);
    leann_backend_close(h);
    return rc;
}

// Continue a build from an existing handle over a caller-staged row block: the one body behind leann_backend_add and
// leann_backend_append[_device].  rows: f32 [nt x src->g.ld] on src's device (selected by the caller), src's rows first, then the new
// ones, zero padded.  *out is a new handle over nt positions that BORROWS the block: the caller keeps it alive or hands it to the
// handle afterwards.  Positions below n_old = src->g.n keep src's levels and lists, whatever made them; positions from n_old on get
// the builder's hash of the position, and upper_off is the prefix sum of that table — which takes src's upper_off to be the prefix sum
// of src's levels (so for every built, opened or compacted handle), the old upper lists then keeping their places in front of the new
// ones.  The stored link distances are recomputed from the rows (link_dist_kernel), the pending area starts empty, and the batched
// insertion goes on from src's entry and max_level in insertion_order(n_old, nt), batches by LEANN_BUILD_BATCH_FRACTION, Vamana
// pruning by the form src recorded and flushing over all positions at the end.  nt == n_old: a copy of src's graph.  efc, alpha, the
// prune form, the reference-ef latch, key offset and device are src's; removals, planes and coalescing are the caller's business.
// src is only read; on an error nothing of the call's stays allocated and *out stays null.
static int continue_build(const leann_backend *src, const float *rows, size_t nt, const char *who, leann_backend **out) {
    *out = nullptr;
    const size_t n_old = src->g.n;
    std::vector<uint8_t> levels(std::max<size_t>(nt, 1), 0);
    uint64_t old_lists = 0;
    if (n_old) {
        std::vector<uint32_t> uo(n_old), want(n_old);
        if (hipMemcpy(levels.data(), src->store.levels, n_old, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(uo.data(), src->g.upper_off, n_old * 4, hipMemcpyDeviceToHost) != hipSuccess) {
            leann_set_error("%s: reading the level tables failed: %s", who, hipGetErrorString(hipGetLastError()));
            return LEANN_ERR_DEVICE;
        }
        old_lists = leann_internal_upper_offsets(levels.data(), n_old, want.data());
        for (size_t i = 0; i < n_old; i++)
            if (uo[i] != want[i]) {
                leann_set_error("%s: upper_off[%zu] is %u where the prefix sum of the levels is %llu; an append keeps the old upper lists in "
                                "place, which needs upper_off to be that prefix sum (re-make the handle with such a table)",
                                who, i, uo[i], (unsigned long long)want[i]);
                return LEANN_ERR_INVALID;
            }
        if (old_lists > src->n_upper_lists) {
            leann_set_error("%s: inconsistent level table: the levels name %llu upper lists, the index holds %llu", who,
                            (unsigned long long)old_lists, (unsigned long long)src->n_upper_lists);
            return LEANN_ERR_INVALID;
        }
    }
    // every allocation of the result is a member of the handle: one leann_backend_close frees whatever a failure leaves behind
    HandlePtr h = leann_internal_new_like(src); // d, ld, M, M0, entry, max_level and the build parameters are src's
    h->g.X = rows; // borrowed
    h->g.n = nt;
    if (int rc = alloc_graph_arrays(h.get(), LEVEL_SEED, levels, n_old)) return rc;
    if (n_old) {
        if (hipMemcpy(h->store.adj0, src->g.adj0, n_old * h->g.M0 * 4, hipMemcpyDeviceToDevice) != hipSuccess ||
            (old_lists && hipMemcpy(h->store.adjU, src->g.adjU, old_lists * h->g.M * 4, hipMemcpyDeviceToDevice) != hipSuccess)) {
            leann_set_error("%s: copying the existing graph failed: %s", who, hipGetErrorString(hipGetLastError()));
            return LEANN_ERR_DEVICE;
        }
    }
    if (nt > n_old)
        if (int rc = build_on_device(h.get(), n_old, 0, true)) return rc;
    *out = h.release();
    return LEANN_OK;
}

// BackendBuilder::add_to_index — src/backend/mod.rs:82-100, hnsw.rs:142-191
extern "C" int leann_backend_add(int backend, const float *vectors, size_t n, size_t dims, size_t start_id,
                                 const char *index_path_stem) {
    if (backend == LEANN_BACKEND_DISKANN) { // mod.rs:93-98
        leann_set_error("DiskANN backend does not support incremental updates. Use --force to rebuild the entire index.");
        return LEANN_ERR_UNSUPPORTED;
    }
    if (backend != LEANN_BACKEND_HNSW || !index_path_stem || (n && !vectors)) {
        leann_set_error("leann_backend_add: invalid arguments");
        return LEANN_ERR_INVALID;
    }
    leann_backend *old = nullptr;
    int rc = leann_backend_open(index_path_stem, backend, dims, "0", &old);
    if (rc) return rc;
    const size_t n_old = old->g.n;
    if (old->g.feat_h) { // a recompute-on index holds encoder inputs, not vectors: appending needs the passages' features, not their embeddings
        leann_set_error("add_to_index: this index stores no vectors (recompute-on); rebuild it from the encoder inputs (leann_recompute_build_index)");
        leann_backend_close(old);
        return LEANN_ERR_UNSUPPORTED;
    }
    if (leann_internal_narrow_rows(old)) { // the builder reads f32 rows, and appending f32 rows to rounded ones would break the file's reproducibility
        leann_set_error("add_to_index: this index stores %s rows; appending is not supported, rebuild it (leann_backend_build_rows) from all the rows",
                        leann_internal_row_name(old));
        leann_backend_close(old);
        return LEANN_ERR_UNSUPPORTED;
    }
    if (start_id != n_old) { // keys are positions (hnsw.rs:178-179): appended ids must continue the sequence
        leann_set_error("add_to_index: start_id %zu does not continue the index (%zu vectors)", start_id, n_old);
        leann_backend_close(old);
        return LEANN_ERR_INVALID;
    }
    // Append: the new rows continue the batched insertion from the existing graph (hnsw.rs:142-191 adds to the loaded index).
    // Levels are a hash of the position, so the first n_old nodes keep their upper-list offsets; the stored link distances
    // the builder prunes with are recomputed (link_dist_kernel).  The same algorithm as a one-shot build of the concatenation on a
    // different batch schedule (the appended rows are permuted among themselves only).
    const size_t ld = old->g.ld, nt = n_old + n;
    DeviceBuf<float> dX; // this call's own: every handle below borrows the rows and is closed before they go
    if (dX.alloc(std::max<size_t>(nt * ld, 4)) ||
        (n_old && hipMemcpy(dX, old->g.X, n_old * ld * 4, hipMemcpyDeviceToDevice) != hipSuccess) ||
        leann_internal_stage_rows(dX + n_old * ld, ld, vectors, dims, dims, n, true) != hipSuccess) {
        leann_set_error("add_to_index: staging %zu rows on the device failed: %s", nt, hipGetErrorString(hipGetLastError()));
        leann_backend_close(old);
        return LEANN_ERR_DEVICE;
    }
    bool same_levels = true; // an index that did not come from this builder (leann_backend_from_arrays + save) has its own level
                             // table; so has a compacted one (compact.hip): its levels moved with the rows to new positions
    if (n_old) {
        std::vector<uint8_t> la(n_old);
        if (hipMemcpy(la.data(), old->store.levels, n_old, hipMemcpyDeviceToHost) != hipSuccess) {
            leann_set_error("add_to_index: reading the level tables failed");
            leann_backend_close(old);
            return LEANN_ERR_DEVICE;
        }
        for (size_t i = 0; i < n_old && same_levels; i++) same_levels = la[i] == (uint8_t)node_level(LEVEL_SEED, i, old->g.M);
    }
    leann_backend *h = nullptr; // borrows dX
    if (!same_levels) { // foreign level table: rebuild over the concatenation (the pre-append behaviour; leann_backend_append continues)
        rc = build_device_guarded(backend, dX, nt, dims, ld, old->g.M, old->efc, 0, 0, 0, &h, false);
    } else {
        try {
            rc = continue_build(old, dX, nt, "add_to_index", &h);
        } catch (const std::exception &e) {
            leann_set_error("add_to_index: %s", e.what());
            rc = LEANN_ERR_DEVICE;
        }
    }
    if (rc == LEANN_OK) rc = leann_internal_carry_removals(old, h, nt); // removals made so far stay; the appended rows are live
    leann_backend_close(old);
    if (rc == LEANN_OK) rc = leann_backend_save(h, index_path_stem);
    leann_backend_close(h);
    return rc;
}

// ---- leann_backend_append[_device]: a NEW handle that continues h's build with n more rows (include/leann_backend.h) ---------------
namespace {
// everything that needs no device, in the header's order; `ld`: the pitch of the new rows
int append_check(const char *who, const leann_backend *h, const float *vectors, size_t n, size_t ld, leann_backend **out) {
    if (!h || !out || (n && !vectors)) {
        leann_set_error("%s: null argument (a handle, the address of the result and, for n > 0, the rows are needed)", who);
        return LEANN_ERR_INVALID;
    }
    if (h->sharded) {
        leann_set_error("%s: not available on a composite handle; append to its last shard (leann_backend_shard), then "
                        "leann_sharded_from_handles over the shards", who);
        return LEANN_ERR_UNSUPPORTED;
    }
    if (h->g.feat_h) {
        leann_set_error("%s: this index stores no vectors (recompute-on); rebuild it from the encoder inputs (leann_recompute_build_index)", who);
        return LEANN_ERR_UNSUPPORTED;
    }
    if (leann_internal_narrow_rows(h)) {
        leann_set_error("%s: this index stores %s rows and the builder reads f32 rows; rebuild it from all the rows (leann_backend_build_rows)", who,
                        leann_internal_row_name(h));
        return LEANN_ERR_UNSUPPORTED;
    }
    if (h->nav_levels) {
        leann_set_error("%s: this Vamana index was built with entry layers (LEANN_VAMANA_NAV=1, an experiment knob); rebuild it "
                        "(leann_backend_build_device) over all the rows", who);
        return LEANN_ERR_UNSUPPORTED;
    }
    if (ld < h->g.d || (ld & 3)) {
        leann_set_error("%s: ld = %zu; the rows need a pitch of at least %u floats (the index's dims) that is a multiple of 4", who, ld, h->g.d);
        return LEANN_ERR_INVALID;
    }
    if ((uint64_t)h->g.n + n >= (1ull << 31)) {
        leann_set_error("%s: %llu + %zu rows reach 2^31 positions; split the index into shards (leann_sharded_from_handles)", who,
                        (unsigned long long)h->g.n, n);
        return LEANN_ERR_INVALID;
    }
    return LEANN_OK;
}

// `vectors`: n rows at pitch `ld` floats, on the host (`on_host`) or on h's device
int append_impl(const char *who, const leann_backend *hc, const float *vectors, size_t n, size_t ld, bool on_host, leann_backend **out) {
    if (out) *out = nullptr;
    if (int rc = append_check(who, hc, vectors, n, ld, out)) return rc;
    if (int rc = leann_internal_check_device(hc->device)) return rc;
    BCHECK(hipSetDevice(hc->device));
    BCHECK(hipDeviceSynchronize());
    const size_t n_old = hc->g.n, nt = n_old + n, gld = hc->g.ld, d = hc->g.d;
    // rows: h's, byte for byte, then the new ones at h's pitch, zero padded
    DeviceBuf<float> rows;
    if (int rc = rows.alloc(std::max<size_t>(nt * gld, 4))) return rc;
    if (n_old) BCHECK(hipMemcpy(rows, hc->g.X, n_old * gld * 4, hipMemcpyDeviceToDevice));
    BCHECK(leann_internal_stage_rows(rows + n_old * gld, gld, vectors, on_host ? d : ld, d, n, on_host)); // (host rows are [n x dims], unpadded)
    leann_backend *raw = nullptr;
    if (int rc = continue_build(hc, rows, nt, who, &raw)) return rc;
    HandlePtr h(raw);
    leann_internal_own_rows(h.get(), std::move(rows)); // the result always owns its rows
    if (int rc = leann_internal_carry_removals(hc, h.get(), nt)) return rc;
    if (int rc = leann_internal_copy_coalescing(hc, h.get())) return rc;
    leann_internal_sync_planes(h.get());
    *out = h.release();
    return LEANN_OK;
}
int append_guarded(const char *who, const leann_backend *h, const float *vectors, size_t n, size_t ld, bool on_host, leann_backend **out) {
    try { // host-side bookkeeping allocates: nothing may be thrown across the C ABI
        return append_impl(who, h, vectors, n, ld, on_host, out);
    } catch (const std::exception &e) {
        if (out) *out = nullptr;
        leann_set_error("%s: %s", who, e.what());
        return LEANN_ERR_DEVICE;
    }
}
} // namespace

extern "C" int leann_backend_append(const leann_backend *h, const float *vectors, size_t n, leann_backend **out) {
    return append_guarded("leann_backend_append", h, vectors, n, h ? (size_t)((h->g.d + 3u) & ~3u) : 0, true, out);
}
extern "C" int leann_backend_append_device(const leann_backend *h, const float *d_vectors, size_t n, size_t ld, leann_backend **out) {
    return append_guarded("leann_backend_append_device", h, d_vectors, n, ld, false, out);
}
