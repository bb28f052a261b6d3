// consolidate.hip — removing passages from a graph index.
//
// leann_backend_remove marks positions as removed (tombstones): nothing moves, positions are never renumbered, and every search
// masks them out (api.hip: leann_internal_search_plain, through leann_internal_live_allow).  While live lists still name removed
// positions the unfiltered walk has to run the filtered kernel; leann_backend_consolidate repairs the graph so that it need not:
//
//   per level, 1. mark    every live node whose list names a removed id goes onto a work list;
//              2. repair  one workgroup per work-list entry p re-links p through its removed neighbours (FreshDiskANN Alg. 4):
//                         C = (N(p) \ D)  ∪  ⋃_{v ∈ N(p) ∩ D} (N(v) \ D),  p itself excluded, N(.) read from a snapshot of the
//                         adjacency taken before the pass (the result does not depend on workgroup order);  dist(p, c) = 1 - <x_p, x_c>;
//                         keys orderable(dist) << 32 | id, ascending, equal keys dropped, the NC nearest kept — C holds up to
//                         width x (width + 1) ids, so it is taken in chunks of NC merged into a running best-NC —; then the builder's
//                         own prune_core<NC> (prune.cuh) with the handle's rule and the list width as the limit;
//              3. clear   lists of removed nodes become empty; a removed entry point is replaced.
//
// The repair kernel is a whole-row gather like the builder's prune: ~|C| x ld x 4 bytes per repaired node for the distances plus the
// NC rows of the Gram matrix.  Lists of nodes that named no removed id are not written at all.
#include "common.cuh"
#include "search.cuh"
#include "internal.h"
#include "prune.cuh"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <sys/stat.h>
#include <vector>

__device__ __forceinline__ bool bit_live(const uint8_t *__restrict__ live, uint32_t id) { return (live[id >> 3] >> (id & 7)) & 1; }

// out[q][b] = allow[q][b] & live[b]; bytes of a row past the bitmap are zeroed.  stride == 0: one bitmap.  out may alias allow.
__global__ void and_live_kernel(uint8_t *out, const uint8_t *allow, const uint8_t *__restrict__ live, size_t nbytes, size_t stride,
                                size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const size_t b = stride ? i % stride : i;
    out[i] = b < nbytes ? (uint8_t)(allow[i] & live[b]) : (uint8_t)0;
}

// list of node v on `level`: level 0 -> adj0 + v * M0; level l >= 1 -> adjU + (upper_off[v] + l - 1) * M
struct LevelLists {
    const uint32_t *upper_off;
    const uint8_t *levels;
    uint32_t level, W; // list width on this level
};
__device__ __forceinline__ size_t list_off(const LevelLists &L, uint32_t v) {
    return L.level == 0 ? (size_t)v * L.W : ((size_t)L.upper_off[v] + (L.level - 1)) * L.W;
}

// 1. mark: live nodes of this level whose list names a removed id -> work list (order immaterial: repairs are independent)
__global__ void mark_kernel(const uint32_t *__restrict__ adj, LevelLists L, const uint8_t *__restrict__ live, uint32_t n,
                            uint32_t *__restrict__ work, uint32_t *__restrict__ n_work) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n || !bit_live(live, p) || L.levels[p] < L.level) return;
    const uint32_t *l = adj + list_off(L, p);
    for (uint32_t j = 0; j < L.W; j++) {
        const uint32_t id = l[j];
        if (id != LEANN_EMPTY && !bit_live(live, id)) {
            work[atomicAdd(n_work, 1u)] = p;
            return;
        }
    }
}
// removed positions still named by a live list of this level: flag[id] = 1
__global__ void pending_kernel(const uint32_t *__restrict__ adj, LevelLists L, const uint8_t *__restrict__ live, uint32_t n,
                               uint8_t *__restrict__ flag) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n || !bit_live(live, p) || L.levels[p] < L.level) return;
    const uint32_t *l = adj + list_off(L, p);
    for (uint32_t j = 0; j < L.W; j++) {
        const uint32_t id = l[j];
        if (id != LEANN_EMPTY && !bit_live(live, id)) flag[id] = 1;
    }
}
__global__ void count_flags_kernel(const uint8_t *__restrict__ flag, uint32_t n, uint32_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool set = i < n && flag[i];
    const unsigned long long m = __ballot(set);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(out, (uint32_t)__popcll(m));
}
// 3. clear: every list of a removed node
__global__ void clear_kernel(uint32_t *__restrict__ adj, LevelLists L, const uint8_t *__restrict__ live, uint32_t n) {
    const uint32_t v = blockIdx.x;
    if (v >= n || bit_live(live, v) || L.levels[v] < L.level) return;
    uint32_t *l = adj + list_off(L, v);
    for (uint32_t j = threadIdx.x; j < L.W; j += blockDim.x) l[j] = LEANN_EMPTY;
}

// 2. repair.  256 threads; NC = 128 for lists of <= 64 ids, 256 for wide graphs (the pools of prune.cuh).
#define CONS_RB 8 // rows whose loads a wave has in flight per 256-float slab
template <int NC>
__device__ __forceinline__ void repair_one(const float *__restrict__ X, uint32_t ld, const uint32_t *__restrict__ old_adj,
                                           uint32_t *__restrict__ new_adj, LevelLists L, const uint8_t *__restrict__ live,
                                           const uint32_t *__restrict__ work, uint32_t n_work, float alpha, uint32_t two_stage) {
    __shared__ __attribute__((aligned(16))) float tri[Pool<NC>::TRI]; // x_p while distances are computed, then the Gram triangle
    __shared__ __attribute__((aligned(16))) float wstage[Pool<NC>::STAGE];
    __shared__ uint64_t skey[2 * NC]; // [0, NC): running best, ascending, unique; [NC, 2 NC): the chunk
    __shared__ uint32_t c_id[NC];
    __shared__ float c_d[NC];
    __shared__ uint32_t s_sel[64 * Pool<NC>::KS];
    __shared__ uint32_t s_src[129]; // p, then its removed neighbours
    __shared__ uint32_t s_cnt, s_nsrc;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t W = L.W;
    const int T = (int)((ld + 255) / 256);
    for (uint32_t wi = blockIdx.x; wi < n_work; wi += gridDim.x) {
        const uint32_t p = work[wi];
        const size_t lp = list_off(L, p);
        if (tid == 0) { s_src[0] = p; s_nsrc = 1; }
        __syncthreads();
        if ((uint32_t)tid < W) {
            const uint32_t id = old_adj[lp + tid];
            if (id != LEANN_EMPTY && !bit_live(live, id)) s_src[atomicAdd(&s_nsrc, 1u)] = id; // <= W of them: s_src holds W + 1 <= 129
        }
        const float *xp = X + (size_t)p * ld;
        for (uint32_t j = 4u * tid; j < ld; j += 1024u) *reinterpret_cast<float4 *>(tri + j) = *reinterpret_cast<const float4 *>(xp + j);
        for (int i = tid; i < NC; i += 256) skey[i] = ~0ull;
        __syncthreads();
        const uint32_t n_slots = s_nsrc * W;
        for (uint32_t c0 = 0; c0 < n_slots; c0 += NC) {
            int any = 0;
            for (int t = tid; t < NC; t += 256) {
                const uint32_t s = c0 + t;
                uint32_t id = LEANN_EMPTY;
                if (s < n_slots) {
                    id = old_adj[list_off(L, s_src[s / W]) + s % W];
                    if (id == p || (id != LEANN_EMPTY && !bit_live(live, id))) id = LEANN_EMPTY;
                }
                c_id[t] = id;
                any |= id != LEANN_EMPTY;
            }
            if (!__syncthreads_or(any)) continue; // (uniform) nothing live in this chunk
            // distances: wave w takes rows [base, base + RB) of every 4 RB; per slab all RB 16-byte loads are issued before the first fma
            for (int base = wave * CONS_RB; base < NC; base += 4 * CONS_RB) {
                uint32_t rid[CONS_RB];
                int live_rows = 0;
#pragma unroll
                for (int r = 0; r < CONS_RB; r++) { rid[r] = c_id[base + r]; live_rows |= rid[r] != LEANN_EMPTY; }
                if (!live_rows) { // (wave-uniform: the ids come from LDS)
                    if (lane < CONS_RB) skey[NC + base + lane] = ~0ull;
                    continue;
                }
                float4 acc[CONS_RB];
#pragma unroll
                for (int r = 0; r < CONS_RB; r++) acc[r] = make_float4(0.f, 0.f, 0.f, 0.f);
                for (int t = 0; t < T; t++) {
                    const uint32_t j = 256u * t + 4u * lane;
                    float4 v[CONS_RB];
#pragma unroll
                    for (int r = 0; r < CONS_RB; r++)
                        v[r] = (rid[r] != LEANN_EMPTY && j < ld) ? *reinterpret_cast<const float4 *>(X + (size_t)rid[r] * ld + j)
                                                                 : make_float4(0.f, 0.f, 0.f, 0.f);
                    const float4 q = j < ld ? *reinterpret_cast<const float4 *>(tri + j) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int r = 0; r < CONS_RB; r++) fma4(acc[r], v[r], q);
                }
#pragma unroll
                for (int r = 0; r < CONS_RB; r++) {
                    const float dot = wave_tree_sum(lane4_sum(acc[r]));
                    if (lane == 0)
                        skey[NC + base + r] = rid[r] != LEANN_EMPTY ? (((uint64_t)f32_orderable(1.0f - dot) << 32) | rid[r]) : ~0ull;
                }
            }
            // merge: sort best ∪ chunk, drop equal neighbours (the same id always carries the same distance), sort again
            bitonic_sort_lds(skey, 2 * NC);
            bool dup[2 * NC / 256];
#pragma unroll
            for (int e = 0; e < 2 * NC / 256; e++) {
                const int i = tid + 256 * e;
                dup[e] = i > 0 && skey[i] != ~0ull && skey[i] == skey[i - 1];
            }
            bool d = false;
#pragma unroll
            for (int e = 0; e < 2 * NC / 256; e++) d = d || dup[e];
            const int any_dup = __syncthreads_or(d);
            if (any_dup) {
#pragma unroll
                for (int e = 0; e < 2 * NC / 256; e++)
                    if (dup[e]) skey[tid + 256 * e] = ~0ull;
                bitonic_sort_lds(skey, 2 * NC);
            }
        }
        __syncthreads();
        int mine = 0;
        for (int i = tid; i < NC; i += 256) {
            const uint64_t k = skey[i];
            mine += k != ~0ull;
            c_id[i] = k != ~0ull ? (uint32_t)k : 0u;
            c_d[i] = k != ~0ull ? orderable_f32((uint32_t)(k >> 32)) : 0.f;
        }
        const uint32_t nc = (uint32_t)__syncthreads_count(mine); // NC <= 256: one key per thread
        uint32_t ns = 0;
        if (nc) ns = prune_core<NC>(X, ld, c_id, c_d, nc, W, alpha, tri, s_sel, &s_cnt, two_stage != 0, wstage);
        for (uint32_t j = tid; j < W; j += 256) new_adj[lp + j] = j < ns ? c_id[s_sel[j]] : LEANN_EMPTY;
        __syncthreads();
    }
}
__global__ void __launch_bounds__(256) repair_kernel(const float *__restrict__ X, uint32_t ld, const uint32_t *__restrict__ old_adj,
                                                     uint32_t *__restrict__ new_adj, LevelLists L, const uint8_t *__restrict__ live,
                                                     const uint32_t *__restrict__ work, uint32_t n_work, float alpha, uint32_t two_stage) {
    repair_one<NCMAX>(X, ld, old_adj, new_adj, L, live, work, n_work, alpha, two_stage);
}
__global__ void __launch_bounds__(256) wide_repair_kernel(const float *__restrict__ X, uint32_t ld, const uint32_t *__restrict__ old_adj,
                                                          uint32_t *__restrict__ new_adj, LevelLists L, const uint8_t *__restrict__ live,
                                                          const uint32_t *__restrict__ work, uint32_t n_work, float alpha,
                                                          uint32_t two_stage) {
    repair_one<NCWIDE>(X, ld, old_adj, new_adj, L, live, work, n_work, alpha, two_stage);
}

#define CCHECK(expr)                                                                                                       \
    do {                                                                                                                   \
        hipError_t _e = (expr);                                                                                            \
        if (_e != hipSuccess) {                                                                                            \
            leann_set_error("remove / consolidate: %s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return LEANN_ERR_DEVICE;                                                                                       \
        }                                                                                                                  \
    } while (0)

static LevelLists level_lists(const leann_backend *h, uint32_t level) {
    LevelLists L;
    L.upper_off = h->g.upper_off;
    L.levels = h->store.levels;
    L.level = level;
    L.W = level == 0 ? h->g.M0 : h->g.M;
    return L;
}

// removed positions a live list (any level) still names
static int count_pending(leann_backend *h, size_t *out) {
    *out = 0;
    const uint32_t n = (uint32_t)h->g.n;
    if (!n || !h->d_live || !h->n_removed) return LEANN_OK;
    DeviceBuf<uint8_t> flag;
    DeviceBuf<uint32_t> cnt;
    if (flag.alloc(n) || cnt.alloc(1)) return LEANN_ERR_DEVICE;
    CCHECK(hipMemset(flag, 0, n));
    CCHECK(hipMemset(cnt, 0, 4));
    for (uint32_t l = 0; l <= h->g.max_level; l++)
        hipLaunchKernelGGL(pending_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, l == 0 ? h->g.adj0 : h->g.adjU, level_lists(h, l),
                           h->d_live, n, flag.p);
    hipLaunchKernelGGL(count_flags_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, flag.p, n, cnt.p);
    CCHECK(hipGetLastError());
    uint32_t c = 0;
    CCHECK(hipMemcpy(&c, cnt, 4, hipMemcpyDeviceToHost));
    *out = c;
    return LEANN_OK;
}

// host bitmap -> device live mask (complement, padding bits zero) + n_pending.  Null-stream work followed by a device synchronisation:
// searches run on non-blocking streams, and remove / consolidate are not concurrent with them.
static int upload_live(leann_backend *h) {
    const size_t n = h->g.n, nbytes = (n + 7) / 8;
    std::vector<uint8_t> live(std::max<size_t>(nbytes, 1));
    for (size_t b = 0; b < nbytes; b++) live[b] = (uint8_t)~h->removed[b];
    if (n & 7) live[nbytes - 1] &= (uint8_t)((1u << (n & 7)) - 1u);
    CCHECK(hipSetDevice(h->device));
    CCHECK(hipDeviceSynchronize());
    if (!h->d_live && h->d_live.alloc(std::max<size_t>(nbytes, 1) + 16)) return LEANN_ERR_DEVICE;
    CCHECK(hipMemcpy(h->d_live, live.data(), nbytes, hipMemcpyHostToDevice));
    if (int rc = count_pending(h, &h->n_pending)) return rc;
    CCHECK(hipDeviceSynchronize());
    return LEANN_OK;
}

int leann_internal_set_removed(leann_backend *h, const uint8_t *bitmap, size_t n_removed) {
    if (h->sharded) { leann_set_error("tombstones are kept per shard"); return LEANN_ERR_UNSUPPORTED; }
    const size_t nbytes = (h->g.n + 7) / 8;
    if (h->d_live) { (void)hipSetDevice(h->device); (void)hipDeviceSynchronize(); h->d_live.reset(); }
    h->removed.assign(bitmap, bitmap + nbytes);
    h->n_removed = n_removed;
    h->n_pending = 0;
    if (!n_removed) { h->removed.clear(); return LEANN_OK; }
    h->removal_epoch++;
    return upload_live(h);
}

int leann_internal_live_allow(leann_backend *h, const uint8_t *d_allow, size_t allow_stride, size_t nq, bool walk, hipStream_t st,
                              const uint8_t **out, size_t *out_stride) {
    *out = d_allow;
    *out_stride = allow_stride;
    if (!h->d_live) return LEANN_OK;
    if (!d_allow) { // the walk needs no mask once no live list names a removed position (unless nothing is live: the entry point itself is removed)
        const bool plain = walk && h->n_pending == 0 && h->n_removed < h->g.n;
        *out = plain ? nullptr : h->d_live;
        *out_stride = 0;
        return LEANN_OK;
    }
    const size_t nbytes = (h->g.n + 7) / 8, total = allow_stride ? allow_stride * nq : nbytes;
    uint8_t *buf = nullptr;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        auto &sc = h->live_scratch[st];
        if (int rc = sc.grow(total)) return rc; // grows to the largest request of the stream, then allocates nothing
        buf = sc;
    }
    hipLaunchKernelGGL(and_live_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, buf, d_allow, h->d_live, nbytes, allow_stride, total);
    CCHECK(hipGetLastError());
    *out = buf;
    return LEANN_OK;
}
// a registered filter's own bitmap, in place (api.hip: leann_backend_filter_create)
int leann_internal_and_live_inplace(const leann_backend *h, uint8_t *d_bitmap) {
    if (!h->d_live || !h->g.n) return LEANN_OK;
    const size_t nbytes = (h->g.n + 7) / 8;
    hipLaunchKernelGGL(and_live_kernel, dim3((unsigned)((nbytes + 255) / 256)), dim3(256), 0, nullptr, d_bitmap, d_bitmap, h->d_live, nbytes, (size_t)0, nbytes);
    CCHECK(hipGetLastError());
    CCHECK(hipDeviceSynchronize());
    return LEANN_OK;
}

// ---- C ABI ---------------------------------------------------------------------------------------------------------------------
static int remove_plain(leann_backend *h, const uint64_t *keys, size_t n, size_t *n_removed) {
    const size_t N = h->g.n, nbytes = (N + 7) / 8;
    for (size_t i = 0; i < n; i++)
        if (keys[i] < h->key_offset || keys[i] - h->key_offset >= N) {
            leann_set_error("leann_backend_remove: unknown key %llu (the index holds keys %llu .. %llu)", (unsigned long long)keys[i],
                            (unsigned long long)h->key_offset, (unsigned long long)(h->key_offset + N) - 1);
            return LEANN_ERR_INVALID;
        }
    if (h->removed.size() != nbytes) h->removed.assign(nbytes, 0);
    size_t fresh = 0;
    for (size_t i = 0; i < n; i++) {
        const size_t pos = (size_t)(keys[i] - h->key_offset);
        if (!((h->removed[pos >> 3] >> (pos & 7)) & 1)) { h->removed[pos >> 3] |= (uint8_t)(1u << (pos & 7)); fresh++; }
    }
    if (n_removed) *n_removed = fresh;
    if (!fresh) return LEANN_OK;
    h->n_removed += fresh;
    h->removal_epoch++;
    return upload_live(h);
}

extern "C" int leann_backend_remove(leann_backend *h, const uint64_t *keys, size_t n, size_t *n_removed) {
    if (n_removed) *n_removed = 0;
    if (!h || (n && !keys)) { leann_set_error("leann_backend_remove: null argument"); return LEANN_ERR_INVALID; }
    try {
        if (!h->sharded) return remove_plain(h, keys, n, n_removed);
        // composite handle: every key goes to the shard that owns its range; nothing is applied unless every key is known
        const size_t G = leann_internal_sharded_count(h->sharded);
        std::vector<std::vector<uint64_t>> per(G);
        for (size_t i = 0; i < n; i++) {
            size_t g = 0;
            for (; g < G; g++) {
                const leann_backend *sh = leann_internal_sharded_shard(h->sharded, g);
                if (sh && keys[i] >= sh->key_offset && keys[i] - sh->key_offset < sh->g.n) break;
            }
            if (g == G) { leann_set_error("leann_backend_remove: unknown key %llu", (unsigned long long)keys[i]); return LEANN_ERR_INVALID; }
            per[g].push_back(keys[i]);
        }
        size_t total = 0;
        for (size_t g = 0; g < G; g++) {
            if (per[g].empty()) continue;
            size_t k = 0;
            if (int rc = remove_plain(leann_internal_sharded_shard(h->sharded, g), per[g].data(), per[g].size(), &k)) return rc;
            total += k;
        }
        (void)hipSetDevice(h->device);
        if (total) h->removal_epoch++;
        if (n_removed) *n_removed = total;
        return LEANN_OK;
    } catch (const std::exception &e) {
        leann_set_error("leann_backend_remove: %s", e.what());
        return LEANN_ERR_DEVICE;
    }
}

extern "C" size_t leann_backend_live_len(const leann_backend *h) {
    if (!h) return 0;
    if (!h->sharded) return (size_t)h->g.n - h->n_removed;
    size_t live = 0;
    for (size_t g = 0; g < leann_internal_sharded_count(h->sharded); g++)
        if (const leann_backend *sh = leann_internal_sharded_shard(h->sharded, g)) live += (size_t)sh->g.n - sh->n_removed;
    return live;
}

extern "C" int leann_backend_removed_bitmap(const leann_backend *h, uint8_t *out, size_t *n_pending) {
    if (!h || !out) { leann_set_error("leann_backend_removed_bitmap: null argument"); return LEANN_ERR_INVALID; }
    const size_t nbytes = (h->g.n + 7) / 8;
    memset(out, 0, nbytes);
    size_t pend = 0;
    if (h->sharded) { // interior shard boundaries are multiples of 64: the per-shard bitmaps concatenate at byte boundaries
        const size_t G = leann_internal_sharded_count(h->sharded);
        for (size_t g = 0; g < G; g++) {
            const leann_backend *sh = leann_internal_sharded_shard(h->sharded, g);
            const uint64_t lo = leann_internal_sharded_lo(h->sharded, g);
            if (!sh || (lo & 7)) { leann_set_error("leann_backend_removed_bitmap: shard %zu does not start at a multiple of 8", g); return LEANN_ERR_UNSUPPORTED; }
            if (!sh->removed.empty()) memcpy(out + lo / 8, sh->removed.data(), sh->removed.size());
            pend += sh->n_pending;
        }
    } else {
        if (!h->removed.empty()) memcpy(out, h->removed.data(), nbytes);
        pend = h->n_pending;
    }
    if (n_pending) *n_pending = pend;
    return LEANN_OK;
}

static int consolidate_plain(leann_backend *h) {
    if (h->g.feat_h) {
        leann_set_error("leann_backend_consolidate: a recompute-on index holds no f32 rows to prune on; its removals stay tombstones");
        return LEANN_ERR_UNSUPPORTED;
    }
    if (leann_internal_narrow_rows(h)) {
        leann_set_error("leann_backend_consolidate: the repair prunes on f32 rows; this index stores %s rows, its removals stay tombstones answered by the filtered walk",
                        leann_internal_row_name(h));
        return LEANN_ERR_UNSUPPORTED;
    }
    if (!h->n_removed || !h->d_live || !h->g.n) return LEANN_OK;
    const uint32_t n = (uint32_t)h->g.n;
    CCHECK(hipSetDevice(h->device));
    CCHECK(hipDeviceSynchronize());
    DeviceBuf<uint32_t> work, cnt, snap;
    const size_t b0 = (size_t)n * h->g.M0 * 4, bU = h->n_upper_lists * (size_t)h->g.M * 4;
    if (work.alloc(n) || cnt.alloc(1) || snap.alloc(std::max<size_t>(std::max(b0, bU), 4) / 4)) return LEANN_ERR_DEVICE;
    const bool wide = std::max(h->g.M0, h->g.M) > 64;
    const float alpha = h->kind == LEANN_BACKEND_DISKANN ? h->alpha : 0.f;
    for (uint32_t l = 0; l <= h->g.max_level; l++) {
        uint32_t *adj = l == 0 ? h->store.adj0 : h->store.adjU;
        const LevelLists L = level_lists(h, l);
        // N(.) is read as it was before this consolidate.  The upper lists share one array and the lists of different levels are
        // disjoint, so the snapshot taken at level 1 serves every level above it.
        if (l <= 1) CCHECK(hipMemcpy(snap, adj, l == 0 ? b0 : bU, hipMemcpyDeviceToDevice));
        CCHECK(hipMemset(cnt, 0, 4));
        hipLaunchKernelGGL(mark_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, adj, L, h->d_live, n, work.p, cnt.p);
        CCHECK(hipGetLastError());
        uint32_t nw = 0;
        CCHECK(hipMemcpy(&nw, cnt, 4, hipMemcpyDeviceToHost));
        if (nw) {
            hipLaunchKernelGGL(wide ? wide_repair_kernel : repair_kernel, dim3(nw), dim3(256), 0, nullptr, h->g.X, h->g.ld, (const uint32_t *)snap.p, adj,
                               L, h->d_live, (const uint32_t *)work.p, nw, alpha, h->two_stage);
            CCHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(clear_kernel, dim3(n), dim3(64), 0, nullptr, adj, L, h->d_live, n);
        CCHECK(hipGetLastError());
        CCHECK(hipDeviceSynchronize());
    }
    // a removed entry point is replaced
    const uint32_t e = h->g.entry;
    if (((h->removed[e >> 3] >> (e & 7)) & 1) && h->n_removed < n) {
        if (h->g.max_level == 0 && h->kind == LEANN_BACKEND_DISKANN) { // the live row nearest to the old medoid's (ties: lower position)
            DeviceBuf<uint64_t> k;
            DeviceBuf<float> d;
            DeviceBuf<uint32_t> c;
            if (k.alloc(1) || d.alloc(1) || c.alloc(1)) return LEANN_ERR_DEVICE;
            if (int rc = leann_internal_filtered_exact(h->g.X, n, h->g.d, h->g.ld, h->g.X + (size_t)e * h->g.ld, 1, 1, h->d_live, 0, 0, k, d, c, nullptr))
                return rc;
            uint64_t key = 0;
            uint32_t got = 0;
            CCHECK(hipMemcpy(&key, k, 8, hipMemcpyDeviceToHost));
            CCHECK(hipMemcpy(&got, c, 4, hipMemcpyDeviceToHost));
            if (got != 1 || key >= n) { leann_set_error("leann_backend_consolidate: no live row found for the entry point"); return LEANN_ERR_DEVICE; }
            h->g.entry = (uint32_t)key;
        } else { // the live node of the highest level, lowest id on ties; max_level follows it down
            std::vector<uint8_t> lv(n);
            CCHECK(hipMemcpy(lv.data(), h->store.levels, n, hipMemcpyDeviceToHost));
            int best_l = -1;
            uint32_t best = 0;
            for (uint32_t v = 0; v < n; v++)
                if (!((h->removed[v >> 3] >> (v & 7)) & 1) && (int)lv[v] > best_l) { best_l = lv[v]; best = v; }
            h->g.entry = best;
            h->g.max_level = std::min<uint32_t>(h->g.max_level, (uint32_t)best_l);
        }
    }
    if (int rc = count_pending(h, &h->n_pending)) return rc;
    CCHECK(hipDeviceSynchronize());
    return LEANN_OK;
}

extern "C" int leann_backend_consolidate(leann_backend *h) {
    if (!h) { leann_set_error("leann_backend_consolidate: null handle"); return LEANN_ERR_INVALID; }
    try {
        if (!h->sharded) return consolidate_plain(h);
        const size_t G = leann_internal_sharded_count(h->sharded);
        int rc = LEANN_OK;
        for (size_t g = 0; g < G && rc == LEANN_OK; g++) {
            leann_backend *sh = leann_internal_sharded_shard(h->sharded, g);
            rc = sh ? consolidate_plain(sh) : (leann_set_error("leann_backend_consolidate: an RCCL group consolidates each rank's own shard handle"), (int)LEANN_ERR_UNSUPPORTED);
        }
        (void)hipSetDevice(h->device);
        return rc;
    } catch (const std::exception &e) {
        leann_set_error("leann_backend_consolidate: %s", e.what());
        return LEANN_ERR_DEVICE;
    }
}

// ---- tombstone sidecar: "<index file minus its extension>.tombstones" ------------------------------------------------------------
//   "LEANNTB1" | u64 n | u64 removed | u64 n_pending | bitmap ceil(n / 8) bytes (bit set = removed, padding bits zero)
// The name drops the index file's extension, so "documents.index" (HNSW) and "documents.diskann" of one stem would share one sidecar:
// a directory holds one backend's index, as the reference's does (meta.backend_name).
std::string leann_internal_tombstone_file(const std::string &index_file) { return leann_internal_with_extension(index_file, "tombstones"); }

extern "C" int leann_tombstones_write(const char *path, const uint8_t *bitmap, uint64_t n, uint64_t n_pending) {
    if (!path || (n && !bitmap)) { leann_set_error("leann_tombstones_write: null argument"); return LEANN_ERR_INVALID; }
    const size_t nbytes = (size_t)((n + 7) / 8);
    uint64_t count = 0;
    for (size_t b = 0; b < nbytes; b++) count += (uint64_t)__builtin_popcount(bitmap[b]);
    if ((n & 7) && (bitmap[nbytes - 1] >> (n & 7))) { leann_set_error("leann_tombstones_write: bits set past position %llu", (unsigned long long)n); return LEANN_ERR_INVALID; }
    const std::string tmp = std::string(path) + ".tmp";
    FILE *f = fopen(tmp.c_str(), "wb");
    if (!f) { leann_set_error("cannot create %s", tmp.c_str()); return LEANN_ERR_IO; }
    const uint64_t hd[3] = {n, count, n_pending};
    bool ok = fwrite("LEANNTB1", 1, 8, f) == 8 && fwrite(hd, 8, 3, f) == 3 && (nbytes == 0 || fwrite(bitmap, 1, nbytes, f) == nbytes);
    ok = (fclose(f) == 0) && ok;
    if (!ok || rename(tmp.c_str(), path) != 0) { (void)remove(tmp.c_str()); leann_set_error("cannot write %s", path); return LEANN_ERR_IO; }
    return LEANN_OK;
}
// bitmap_out: ceil(n_expected / 8) bytes.  LEANN_ERR_NOT_FOUND: no such file (not an error for an index without removals).
extern "C" int leann_tombstones_read(const char *path, uint64_t n_expected, uint8_t *bitmap_out, uint64_t *n_removed, uint64_t *n_pending) {
    if (!path || !bitmap_out) { leann_set_error("leann_tombstones_read: null argument"); return LEANN_ERR_INVALID; }
    FILE *f = fopen(path, "rb");
    if (!f) { leann_set_error("cannot open %s", path); return LEANN_ERR_NOT_FOUND; }
    auto bad = [&](const char *why) {
        fclose(f);
        leann_set_error("Failed to load tombstones: %s in %s", why, path);
        return (int)LEANN_ERR_FORMAT;
    };
    struct stat stt{};
    if (fstat(fileno(f), &stt) != 0) return bad("cannot stat");
    char magic[8];
    uint64_t hd[3];
    if (fread(magic, 1, 8, f) != 8 || fread(hd, 8, 3, f) != 3 || memcmp(magic, "LEANNTB1", 8) != 0) return bad("bad magic/header");
    if (hd[0] != n_expected) return bad("the row count differs from the index's");
    const size_t nbytes = (size_t)((n_expected + 7) / 8);
    if ((uint64_t)stt.st_size != 32 + (uint64_t)nbytes) return bad("file length does not match the header (truncated or corrupt)");
    if (nbytes && fread(bitmap_out, 1, nbytes, f) != nbytes) return bad("truncated file");
    uint64_t count = 0;
    for (size_t b = 0; b < nbytes; b++) count += (uint64_t)__builtin_popcount(bitmap_out[b]);
    if (count != hd[1]) return bad("the removal count does not match the bitmap");
    if ((n_expected & 7) && (bitmap_out[nbytes - 1] >> (n_expected & 7))) return bad("padding bits are set");
    if (hd[2] > hd[1]) return bad("more pending removals than removals");
    fclose(f);
    if (n_removed) *n_removed = hd[1];
    if (n_pending) *n_pending = hd[2];
    return LEANN_OK;
}

int leann_internal_tombstones_save(const leann_backend *h, const std::string &index_file) {
    const std::string path = leann_internal_tombstone_file(index_file);
    if (!h->n_removed) { (void)remove(path.c_str()); return LEANN_OK; } // nothing removed: a stale sidecar must not survive
    return leann_tombstones_write(path.c_str(), h->removed.data(), h->g.n, h->n_pending);
}
int leann_internal_tombstones_load(leann_backend *h, const std::string &index_file) {
    const std::string path = leann_internal_tombstone_file(index_file);
    struct stat stt{};
    if (stat(path.c_str(), &stt) != 0) return LEANN_OK;
    std::vector<uint8_t> bm(std::max<size_t>((h->g.n + 7) / 8, 1));
    uint64_t count = 0, pend = 0;
    if (int rc = leann_tombstones_read(path.c_str(), h->g.n, bm.data(), &count, &pend)) return rc == LEANN_ERR_NOT_FOUND ? (int)LEANN_ERR_IO : rc;
    return leann_internal_set_removed(h, bm.data(), (size_t)count); // (n_pending is counted again on the device)
}

// file twin: open -> remove -> consolidate -> save
extern "C" int leann_backend_remove_from_index(int backend, const uint64_t *keys, size_t n, size_t dims, const char *index_path_stem) {
    if (!index_path_stem || (n && !keys)) { leann_set_error("leann_backend_remove_from_index: null argument"); return LEANN_ERR_INVALID; }
    leann_backend *h = nullptr;
    int rc = leann_backend_open(index_path_stem, backend, dims, "0", &h);
    if (rc) return rc;
    if (leann_internal_narrow_rows(h)) { // its consolidate step needs f32 rows: refused before anything changes
        leann_set_error("leann_backend_remove_from_index: not available on an index of %s rows (no graph repair); open it, leann_backend_remove, leann_backend_save: the removals stay tombstones",
                        leann_internal_row_name(h));
        leann_backend_close(h);
        return LEANN_ERR_UNSUPPORTED;
    }
    rc = leann_backend_remove(h, keys, n, nullptr);
    if (rc == LEANN_OK && !h->g.feat_h) rc = leann_backend_consolidate(h); // (recompute-on: the removals stay tombstones)
    if (rc == LEANN_OK) rc = leann_backend_save(h, index_path_stem);
    leann_backend_close(h);
    return rc;
}
