// search.cuh — on-GPU graph traversal for HNSW (level descent + ef beam) and Vamana (single level,
// medoid entry).  Replaces the arithmetic behind
//     HnswSearcher::search     src/backend/hnsw.rs:79-88   (usearch::Index::search, out of tree)
//     DiskAnnSearcher::search  src/backend/diskann.rs:47-62 (diskann_rs search_with_dists, out of tree)
// Restated algorithm: oracle/oracle.c (search_layer_heap / search_layer_list / graph_search_ctx).
//
// Mapping: one workgroup (NW waves of 64) per query.
//   * query vector: registers of every wave (lane l holds elements 256t+4l..+3), loaded once;
//   * result/candidate beam W: sorted u64 keys in LDS, double buffered, merged by rank;
//   * visited set: open-addressing hash table in LDS; a query that outgrows it migrates, mid-search, to a pooled
//     table in HBM (generation-tagged slots touched only by atomics) and continues;
//   * per hop: wave 0 reads the adjacency list (LW neighbour ids per lane: ids l and 64 + l) and filters it through
//     the visited table; the not-yet-seen rows are dealt round-robin to the NW waves, each wave
//     streams a whole row per instruction group (64 lanes x 16 B = 1 KiB coalesced), R rows in
//     flight, and reduces with the canonical wave tree (common.cuh);
//   * merge: one work item per old / new entry ranks itself against the new keys with pipelined 16-byte LDS scans
//     and scatters into the other W buffer; a wave-level min picks the next candidate;
//   * filtered search (allow-bitmap): same traversal; a second sorted list R in LDS keeps the k best
//     ALLOWED keys among everything evaluated on the target level (top-k of a set: order independent, so again
//     bit-identical to the oracle's collect-sort-truncate);
//   * exactly one candidate is expanded per step, in the same order as the sequential algorithm,
//     so ids AND distances are bit-identical to the oracle.
#pragma once
#include "common.cuh"
#include "row_screen.h"
#include "search_plan.h"

struct GraphView {
    const float *X;            // [n x ld] rows, 16-byte aligned, zero padded
    const uint32_t *adj0;      // [n x M0] level-0 neighbours, LEANN_EMPTY padded
    const uint32_t *adjU;      // [n_upper_lists x M] upper-level neighbour lists
    const uint32_t *upper_off; // [n] first upper list of a node (list of level l at upper_off+l-1)
    uint64_t n;
    uint32_t d, ld, M, M0, max_level, entry;
    // recompute-on graph search (no stored vectors): X points at feature rows instead —
    // [feat_h bf16 features][f32 ||W^T f||][pad], `row_bytes` apart; the query side is g = W q (feat_h f32) and
    // dist = 1 - <f, g> / ||W^T f||  ==  1 - <l2norm(W^T f), q>.  feat_h == 0: plain f32 rows.
    uint32_t feat_h, row_bytes;
    // Rows of exactly 256 features live SPLIT on the device: X = [n x 512 B] of features (row_bytes = 512: every row is four whole,
    // aligned 128-B lines) and `norms` = [n] f32.  With the norm inline a 520-B row touches 5.06 lines on average — 20 % of the
    // fabric traffic was padding (PMC 1.20 x the algorithmic bytes, profiles/r02_other_kernels.md).  Files, exports and the oracle keep
    // the inline form (interleaved on the way out); null: inline norm behind the features.
    const float *norms;
};

// Pools of visited tables in HBM for the rare query whose LDS table fills up.  Pool 1: GPOOL_TABLES tables of
// 2^GPOOL_BITS u64 slots {generation:32 | id:32}.  Never cleared: a slot whose generation differs
// from the owner's current one is empty.  Only atomics touch it, so hand-over between workgroups
// on different XCDs needs no fence.  A query that fills even its pool-1 table (> 49 152 nodes visited on one level:
// beams of ~1 000 and more) moves on to pool 2: a few tables sized by the host to hold EVERY node of the index at 75 % load
// (api.hip:ensure_gpool), so a search can never run out of visited-set space; the `aborted` exit below is a defensive path
// (reported as stat 3 and turned into LEANN_ERR_OVERFLOW by the host entry points; reachable only through the debug knobs).
#define GPOOL_TABLES 1024u
#define GPOOL_BITS 16u

struct SearchArgs {
    const float *queries;     // [nq x ldq] (ignored when q_rows != nullptr)
    const uint32_t *q_rows;   // optional: query i is base row q_rows[i] (index construction)
    uint32_t ldq, nq, k, ef, target_level;
    uint32_t hash_bits;       // LDS visited table = 1 << hash_bits slots
    uint64_t key_offset;
    uint64_t *out_keys;       // [nq x k]
    float *out_dists;         // [nq x k]
    uint32_t *out_counts;     // [nq]
    uint32_t *out_stats;      // [nq x 4] evals, hops0, hopsU, visited-set level (0 LDS, 1 / 2 HBM pool, 3 = overflowed: empty result)  (optional)
    uint64_t *out_expanded;   // optional [nq x exp_cap]: (orderable(dist) << 32 | id) of every node expanded on the
    uint32_t *out_nexp;       //          target level, in expansion order (Vamana's visited set V), and its count
    uint32_t exp_cap;
    unsigned long long *gpool; // [gpool_tables << gpool_bits]
    uint32_t *gpool_lock;     // [gpool_tables] 0 = free
    uint32_t *gpool_ctr;      // [0] acquire ticket (pool 1), [1] generation counter, [2] acquire ticket (pool 2)
    uint32_t gpool_bits, gpool_tables;
    unsigned long long *gpool2; // second-level pool (null: the index is small enough for pool 1 to hold all of it)
    uint32_t *gpool2_lock;
    uint32_t gpool2_bits, gpool2_tables;
    const uint8_t *allow;     // filtered kernels only: bitmap over local positions (bit i of byte i >> 3) ...
    uint64_t allow_stride;    // ... of query i at allow + i * allow_stride (0: one bitmap shared by the batch)
    // Row screen (beam_search_screen_kernel only; row_screen.h): the f32 rows a second time as two planes of 16-bit halves,
    // [n x ldp] u16 each in rs_plane_pos order, and two running totals {rows ruled out on the hi plane alone, rows read in full}.
    // Behind every older field, so no other kernel's argument offsets move.
    const uint16_t *x_hi, *x_lo;
    uint32_t ldp;
    unsigned long long *screen_ctr;
};

// The traversal kernels all take (GraphView g, SearchArgs a) by value.  Two dozen of `a`'s fields are needed only by rare paths (visited
// set migration, expansion trace) or once at the end (outputs); read through the by-value struct they are loaded at kernel entry and
// stay live — in scalar registers the hop loop is short of (it spilled 70 of them into vector lanes) — to the last line.  Read from
// the kernel-argument segment at the point of use they cost one scalar load there and nothing in between.
static_assert(alignof(SearchArgs) == 8 && alignof(GraphView) == 8, "lazy_search_args assumes `a` sits at the 8-byte aligned offset behind `g`");
__device__ __forceinline__ const __attribute__((address_space(4))) SearchArgs *lazy_search_args() {
    typedef const __attribute__((address_space(4))) char *kptr;
    return (const __attribute__((address_space(4))) SearchArgs *)((kptr)__builtin_amdgcn_kernarg_segment_ptr() +
                                                                  ((sizeof(GraphView) + 7) & ~(size_t)7));
}

// A value every lane read from the same LDS word: tell the compiler it is uniform, so that it and everything derived from it (beam
// size, buffer pointers, loop bounds) live in scalar registers instead of one vector register each.
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

__device__ __forceinline__ uint32_t vis_hash(uint32_t id, uint32_t bits) {
    return (id * 0x9E3779B1u) >> (32 - bits);
}

__device__ __forceinline__ bool vis_insert_lds(uint32_t *tab, uint32_t bits, uint32_t id) {
    const uint32_t mask = (1u << bits) - 1u;
    uint32_t h = vis_hash(id, bits);
    for (;;) {
        uint32_t old = atomicCAS(&tab[h], LEANN_EMPTY, id);
        if (old == LEANN_EMPTY) return true;
        if (old == id) return false;
        h = (h + 1) & mask;
    }
}
__device__ __forceinline__ bool vis_insert_hbm(unsigned long long *tab, uint32_t bits, uint32_t gen, uint32_t id) {
    const uint32_t mask = (1u << bits) - 1u;
    uint32_t h = vis_hash(id, bits);
    const unsigned long long mine = ((unsigned long long)gen << 32) | id;
    for (;;) {
        unsigned long long cur = __hip_atomic_load(&tab[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((uint32_t)(cur >> 32) != gen) { // stale generation == empty
            unsigned long long prev = atomicCAS(&tab[h], cur, mine);
            if (prev == cur) return true;
            continue; // somebody of this workgroup took the slot: look at it again
        }
        if ((uint32_t)cur == id) return false;
        h = (h + 1) & mask;
    }
}

// ---- distance of up to R rows per wave, all loads issued before the first use -----------------
template <int T, int R>
__device__ __forceinline__ void wave_dist_rows(const float4 (&q)[T], const float *__restrict__ X, uint32_t ld,
                                               const uint32_t (&ids)[R], int nrows, int lane, float (&out)[R]) {
    float4 v[R][T];
#pragma unroll
    for (int r = 0; r < R; r++) {
        if (r < nrows) {
            const float *row = X + (size_t)ids[r] * ld;
#pragma unroll
            for (int t = 0; t < T; t++) v[r][t] = row_load4(row, ld, t, lane);
        }
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
        if (r < nrows) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int t = 0; t < T; t++) fma4(acc, q[t], v[r][t]);
            out[r] = 1.0f - wave_tree_sum(lane4_sum(acc));
        }
    }
}

// ---- the same rows through the split planes (row_screen.h): hi halves first, lo halves only for rows the bound cannot rule out ----
// Lane l's halves of chunk t as {e0 | e1 << 16, e2 | e3 << 16}: one 16-byte load per interleaved 512-element block, 8 bytes per
// chunk of the tail (rs_plane_pos).
__device__ __forceinline__ uint2 plane_tail_load(const uint16_t *__restrict__ row, uint32_t ldp, int c, int lane) {
    const uint32_t j = 256u * c + 4u * lane;
    return j < ldp ? *reinterpret_cast<const uint2 *>(row + j) : make_uint2(0u, 0u);
}
template <int T>
__device__ __forceinline__ void plane_row_load(const uint16_t *__restrict__ row, uint32_t ldp, int lane, uint2 (&h)[T]) {
#pragma unroll
    for (int p = 0; p < T / 2; p++) {
        if (512u * (uint32_t)(p + 1) <= ldp) {
            const uint4 v = *reinterpret_cast<const uint4 *>(row + 512 * p + 8 * lane);
            h[2 * p] = make_uint2(v.x, v.y);
            h[2 * p + 1] = make_uint2(v.z, v.w);
        } else {
            h[2 * p] = plane_tail_load(row, ldp, 2 * p, lane);
            h[2 * p + 1] = plane_tail_load(row, ldp, 2 * p + 1, lane);
        }
    }
    if (T & 1) h[T - 1] = plane_tail_load(row, ldp, T - 1, lane);
}
// `armed`: the beam is full and `worst` is the distance of its last entry.  out[r] = the canonical distance, bit for bit, of every row
// read in full; a lower bound on it, strictly above `worst`, of a row ruled out (bit r of the returned mask).
template <int T, int R>
__device__ __forceinline__ uint32_t wave_dist_rows_screen(const float4 (&q)[T], const uint16_t *__restrict__ Xhi, const uint16_t *__restrict__ Xlo,
                                                          uint32_t ldp, const uint32_t (&ids)[R], int nrows, int lane, bool armed, float worst,
                                                          float E, float (&out)[R]) {
    uint2 h[R][T], l[R][T];
#pragma unroll
    for (int r = 0; r < R; r++)
        if (r < nrows) plane_row_load<T>(Xhi + (size_t)ids[r] * ldp, ldp, lane, h[r]);
    uint32_t ruled = 0;
#pragma unroll
    for (int r = 0; r < R; r++) {
        if (r < nrows) {
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f), a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int t = 0; t < T; t++) {
                float4 x;
                x.x = __uint_as_float(h[r][t].x << 16);
                x.y = __uint_as_float(h[r][t].x & 0xFFFF0000u);
                x.z = __uint_as_float(h[r][t].y << 16);
                x.w = __uint_as_float(h[r][t].y & 0xFFFF0000u);
                fma4(s, q[t], x);
                a.x = fmaf(fabsf(q[t].x), fabsf(x.x), a.x);
                a.y = fmaf(fabsf(q[t].y), fabsf(x.y), a.y);
                a.z = fmaf(fabsf(q[t].z), fabsf(x.z), a.z);
                a.w = fmaf(fabsf(q[t].w), fabsf(x.w), a.w);
            }
            const float lb = rs_lower_bound(wave_tree_sum(rs_lane_bound(lane4_sum(s), lane4_sum(a))), E);
            out[r] = lb;
            if (armed && lb > worst) ruled |= 1u << r; // (false for a NaN on either side)
        }
    }
#pragma unroll
    for (int r = 0; r < R; r++)
        if (r < nrows && !((ruled >> r) & 1u)) plane_row_load<T>(Xlo + (size_t)ids[r] * ldp, ldp, lane, l[r]);
#pragma unroll
    for (int r = 0; r < R; r++) {
        if (r < nrows && !((ruled >> r) & 1u)) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int t = 0; t < T; t++) {
                float4 x;
                x.x = __uint_as_float((h[r][t].x << 16) | (l[r][t].x & 0xFFFFu));
                x.y = __uint_as_float((h[r][t].x & 0xFFFF0000u) | (l[r][t].x >> 16));
                x.z = __uint_as_float((h[r][t].y << 16) | (l[r][t].y & 0xFFFFu));
                x.w = __uint_as_float((h[r][t].y & 0xFFFF0000u) | (l[r][t].y >> 16));
                fma4(acc, q[t], x);
            }
            out[r] = 1.0f - wave_tree_sum(lane4_sum(acc));
        }
    }
    return ruled;
}

// ---- the wide form of the screen (768-d rows, beam_search_screen_kernel<3, R>): the two steps above as two passes over a hop's rows ----
// H rows per wave go through their hi planes in ONE round trip; what the bound cannot rule out is read afterwards as whole rows, hi and
// lo together, R at a time.  A hop of up to NW * H rows is then two dependent round trips where R rows per round made it four.  The hi
// halves of the survivors are not kept (H rows of them next to the lo halves do not fit into the 128 registers the kernel is held to:
// DESIGN.md §3); their lines were fetched a moment earlier by the same CU, so the second read of them is served by the caches.
// H: the largest at which the kernel keeps 128 VGPRs, four workgroups per CU and no more scratch than the R-rows-per-round form had.
#ifndef LEANN_SCREEN_H3
#define LEANN_SCREEN_H3 7
#endif
// Hi pass over rows j0, j0 + NW, .. (at most H of them below n_new) of the hop's unseen ids `snew`, the beam full and `worst` the
// distance of its last entry.  lb as in wave_dist_rows_screen, bit for bit.  A row ruled out (lb > worst; false for a NaN on either
// side) gets its key make_key(lb, id) written at once; the others come back as a wave-uniform mask, bit r = row j0 + r * NW.
template <int T, int H, int NW>
__device__ __forceinline__ uint32_t wave_screen_hi_rows(const float4 (&q)[T], const uint16_t *__restrict__ Xhi, uint32_t ldp,
                                                        const uint32_t *snew, uint64_t *skey, uint32_t j0, uint32_t n_new, int lane,
                                                        float worst, float E) {
    uint2 h[H][T];
#pragma unroll
    for (int r = 0; r < H; r++) {
        if (j0 + r * NW < n_new) {
            const uint32_t id = uni(snew[j0 + r * NW]);
            plane_row_load<T>(Xhi + (size_t)id * ldp, ldp, lane, h[r]);
        }
    }
    uint32_t surv = 0;
#pragma unroll
    for (int r = 0; r < H; r++) {
        if (j0 + r * NW < n_new) {
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f), a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int t = 0; t < T; t++) {
                float4 x;
                x.x = __uint_as_float(h[r][t].x << 16);
                x.y = __uint_as_float(h[r][t].x & 0xFFFF0000u);
                x.z = __uint_as_float(h[r][t].y << 16);
                x.w = __uint_as_float(h[r][t].y & 0xFFFF0000u);
                fma4(s, q[t], x);
                a.x = fmaf(fabsf(q[t].x), fabsf(x.x), a.x);
                a.y = fmaf(fabsf(q[t].y), fabsf(x.y), a.y);
                a.z = fmaf(fabsf(q[t].z), fabsf(x.z), a.z);
                a.w = fmaf(fabsf(q[t].w), fabsf(x.w), a.w);
            }
            const float lb = rs_lower_bound(wave_tree_sum(rs_lane_bound(lane4_sum(s), lane4_sum(a))), E);
            if (lb > worst) {
                if (lane == 0) skey[j0 + r * NW] = make_key(lb, snew[j0 + r * NW]);
            } else {
                surv |= 1u << r;
            }
        }
    }
    return uni(surv);
}
// Survivor pass: the rows j0 + b * NW, b the set bits of the wave-uniform `surv`, read whole — both planes in one round trip, R rows in
// flight — and their canonical distances (the chain of wave_dist_rows_screen's second step, bit for bit) written as keys.  Each
// round takes the lowest R set bits, once for the loads and once more for the sums, and reads the ids from `snew` by index both times:
// arrays of positions and ids filled under `if (m)` cost the kernel 36 B of stack per lane that nothing ever touches.
template <int T, int R, int NW>
__device__ __forceinline__ void wave_dist_rows_planes(const float4 (&q)[T], const uint16_t *__restrict__ Xhi, const uint16_t *__restrict__ Xlo,
                                                      uint32_t ldp, const uint32_t *snew, uint64_t *skey, uint32_t j0, uint32_t surv, int lane) {
    while (surv) {
        uint2 h[R][T], l[R][T];
        uint32_t m = surv;
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (m) {
                const uint32_t id = uni(snew[j0 + (uint32_t)__builtin_ctz(m) * NW]);
                m &= m - 1u;
                plane_row_load<T>(Xhi + (size_t)id * ldp, ldp, lane, h[r]);
                plane_row_load<T>(Xlo + (size_t)id * ldp, ldp, lane, l[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (surv) {
                const uint32_t j = j0 + (uint32_t)__builtin_ctz(surv) * NW;
                surv &= surv - 1u;
                float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int t = 0; t < T; t++) {
                    float4 x;
                    x.x = __uint_as_float((h[r][t].x << 16) | (l[r][t].x & 0xFFFFu));
                    x.y = __uint_as_float((h[r][t].x & 0xFFFF0000u) | (l[r][t].x >> 16));
                    x.z = __uint_as_float((h[r][t].y << 16) | (l[r][t].y & 0xFFFFu));
                    x.w = __uint_as_float((h[r][t].y & 0xFFFF0000u) | (l[r][t].y >> 16));
                    fma4(acc, q[t], x);
                }
                const float dist = 1.0f - wave_tree_sum(lane4_sum(acc));
                if (lane == 0) skey[j] = make_key(dist, snew[j]);
            }
        }
    }
}

// Same for bf16 feature rows with the inline norm (recompute-on mode).  Lane l owns elements 256t+4l..+3 again
// (one 8-byte load per chunk), so the canonical accumulation order is unchanged; only the operands differ.
template <int T, int R>
__device__ __forceinline__ void wave_dist_rows_feat(const float4 (&q)[T], const char *__restrict__ Xb, uint32_t row_bytes,
                                                    uint32_t h, const uint32_t (&ids)[R], int nrows, int lane, float (&out)[R],
                                                    const float *__restrict__ norms = nullptr) {
    uint2 v[R][T];
    float nrm[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        if (r < nrows) {
            const char *row = Xb + (size_t)ids[r] * row_bytes;
#pragma unroll
            for (int t = 0; t < T; t++) {
                const uint32_t j = 256u * t + 4u * lane;
                v[r][t] = j < h ? *reinterpret_cast<const uint2 *>(row + 2 * (size_t)j) : make_uint2(0u, 0u);
            }
            nrm[r] = norms ? norms[ids[r]] : *reinterpret_cast<const float *>(row + 2 * (size_t)h);
        }
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
        if (r < nrows) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int t = 0; t < T; t++) {
                float4 x;
                x.x = __uint_as_float(v[r][t].x << 16);
                x.y = __uint_as_float(v[r][t].x & 0xFFFF0000u);
                x.z = __uint_as_float(v[r][t].y << 16);
                x.w = __uint_as_float(v[r][t].y & 0xFFFF0000u);
                fma4(acc, q[t], x);
            }
            out[r] = 1.0f - wave_tree_sum(lane4_sum(acc)) / nrm[r];
        }
    }
}

// bf16 rows (LEANN_ROWS_BF16, rows_bf16.hip): the stored row IS bf16, [n x ldb] u16 in rs_plane_pos order (ldb: dims rounded up to 64
// elements — whole 128-B lines, zero padded), so a lane's eight halves of a 512-element block come in ONE 16-byte load
// (plane_row_load).  Widened exactly (b << 16) in registers and summed in the canonical order — lane l owns elements 256t+4l..+3,
// fma4 over t ascending, lane4_sum, wave_tree_sum, 1 - sum — so the distance is bit for bit the f32 kernels' on the widened rows.
template <int T, int R>
__device__ __forceinline__ void wave_dist_rows_bf16(const float4 (&q)[T], const uint16_t *__restrict__ Xb, uint32_t ldb,
                                                    const uint32_t (&ids)[R], int nrows, int lane, float (&out)[R]) {
    uint2 v[R][T];
#pragma unroll
    for (int r = 0; r < R; r++)
        if (r < nrows) plane_row_load<T>(Xb + (size_t)ids[r] * ldb, ldb, lane, v[r]);
#pragma unroll
    for (int r = 0; r < R; r++) {
        if (r < nrows) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int t = 0; t < T; t++) {
                float4 x;
                x.x = __uint_as_float(v[r][t].x << 16);
                x.y = __uint_as_float(v[r][t].x & 0xFFFF0000u);
                x.z = __uint_as_float(v[r][t].y << 16);
                x.w = __uint_as_float(v[r][t].y & 0xFFFF0000u);
                fma4(acc, q[t], x);
            }
            out[r] = 1.0f - wave_tree_sum(lane4_sum(acc));
        }
    }
}

// int8 rows (LEANN_ROWS_I8, rows_i8.hip): the stored row is int8 codes, [n x ldb] bytes in i8_row_pos order (i8_rows.h; ldb: dims rounded
// up to 128 — whole 128-B lines, zero padded), so a lane's sixteen codes of a 1 024-element block (four chunks) come in ONE 16-byte load,
// those of a 512-element tail in one 8-byte load, and the rest in 4 bytes per chunk.  The column scales 2^-e_j are applied to the QUERY
// once (beam_search_one stages q'_j = q_j 2^-e_j, exact), so a row costs one conversion and one fmaf per element: q'_j c_ij is the
// real number q_j Xq_ij, and the canonical order — lane l owns elements 256t+4l..+3, fma4 over t ascending, lane4_sum, wave_tree_sum,
// 1 - sum — rounds it exactly as the f32 kernels do on the dequantised rows Xq.
__device__ __forceinline__ uint32_t i8_tail_load(const int8_t *__restrict__ row, uint32_t ldb, int c, int lane) {
    const uint32_t j = 256u * c + 4u * lane;
    return j < ldb ? *reinterpret_cast<const uint32_t *>(row + j) : 0u;
}
template <int T>
__device__ __forceinline__ void i8_row_load(const int8_t *__restrict__ row, uint32_t ldb, int lane, uint32_t (&v)[T]) {
#pragma unroll
    for (int b = 0; b < (T + 3) / 4; b++) {
        const int c = 4 * b;
        if (c + 4 <= T && 1024u * (uint32_t)(b + 1) <= ldb) {
            const uint4 w = *reinterpret_cast<const uint4 *>(row + 1024 * b + 16 * lane);
            v[c] = w.x; v[c + 1] = w.y; v[c + 2] = w.z; v[c + 3] = w.w;
        } else { // the tail (< 1 024 elements): a 512-element pair where it fits, then element order
            if (c + 2 <= T && 1024u * (uint32_t)b + 512u <= ldb) {
                const uint2 w = *reinterpret_cast<const uint2 *>(row + 1024 * b + 8 * lane);
                v[c] = w.x; v[c + 1] = w.y;
            } else {
                v[c] = i8_tail_load(row, ldb, c, lane);
                if (c + 1 < T) v[c + 1] = i8_tail_load(row, ldb, c + 1, lane);
            }
            if (c + 2 < T) v[c + 2] = i8_tail_load(row, ldb, c + 2, lane);
            if (c + 3 < T) v[c + 3] = i8_tail_load(row, ldb, c + 3, lane);
        }
    }
}
template <int T, int R>
__device__ __forceinline__ void wave_dist_rows_i8(const float4 (&q)[T], const int8_t *__restrict__ Xb, uint32_t ldb,
                                                  const uint32_t (&ids)[R], int nrows, int lane, float (&out)[R]) {
    uint32_t v[R][T];
#pragma unroll
    for (int r = 0; r < R; r++)
        if (r < nrows) i8_row_load<T>(Xb + (size_t)ids[r] * ldb, ldb, lane, v[r]);
#pragma unroll
    for (int r = 0; r < R; r++) {
        if (r < nrows) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int t = 0; t < T; t++) {
                float4 x;
                x.x = (float)(int8_t)v[r][t];
                x.y = (float)(int8_t)(v[r][t] >> 8);
                x.z = (float)(int8_t)(v[r][t] >> 16);
                x.w = (float)((int32_t)v[r][t] >> 24);
                fma4(acc, q[t], x);
            }
            out[r] = 1.0f - wave_tree_sum(lane4_sum(acc));
        }
    }
}

// Recompute-on rows of exactly 256 bf16 features (+ inline norm), FOUR passages per wave instruction: the 16 lanes of a DPP row share a
// passage, lane m of them owns elements 8m..8m+7 and 128+8m..128+8m+7 (two 16-byte loads; each instruction reads a contiguous 256-B
// half of four rows), and one pass of the DPP ladder reduces four rows at once — against one row per 8-byte wave load and one
// six-step ladder per row above.  G such groups in flight per wave.  The sum is the SAME balanced tree over the 64 four-element
// partials (partial v = elements 4v..4v+3, lane m holds partials 2m, 2m+1, 32+2m, 32+2m+1): level 1 and level 6 are additions inside
// the lane, levels 2-5 run on the row's DPP ladder — every pairing is wave_tree_sum's, so the distances are bit-identical.
// Results (and the norm load) live in lane 15 of each DPP row.
typedef uint32_t u32x4_a8 __attribute__((ext_vector_type(4), aligned(8)));
__device__ __forceinline__ float feat8_partial_pair(const float (&q)[8], const u32x4_a8 v) {
    float4 lo, hi;
    lo.x = fmaf(q[0], __uint_as_float(v.x << 16), 0.f);
    lo.y = fmaf(q[1], __uint_as_float(v.x & 0xFFFF0000u), 0.f);
    lo.z = fmaf(q[2], __uint_as_float(v.y << 16), 0.f);
    lo.w = fmaf(q[3], __uint_as_float(v.y & 0xFFFF0000u), 0.f);
    hi.x = fmaf(q[4], __uint_as_float(v.z << 16), 0.f);
    hi.y = fmaf(q[5], __uint_as_float(v.z & 0xFFFF0000u), 0.f);
    hi.z = fmaf(q[6], __uint_as_float(v.w << 16), 0.f);
    hi.w = fmaf(q[7], __uint_as_float(v.w & 0xFFFF0000u), 0.f);
    return lane4_sum(lo) + lane4_sum(hi); // level 1: partials 2m and 2m + 1
}
template <int G>
__device__ __forceinline__ void group_dist_rows_feat256(const float (&qa)[8], const float (&qb)[8], const char *__restrict__ Xb,
                                                        uint32_t row_bytes, const uint32_t (&id)[G], const bool (&valid)[G], int lane,
                                                        float (&out)[G], const float *__restrict__ norms) {
    const int m = lane & 15;
    u32x4_a8 va[G], vb[G];
    float nrm[G];
#pragma unroll
    for (int g = 0; g < G; g++) {
        va[g] = vb[g] = u32x4_a8{0u, 0u, 0u, 0u};
        nrm[g] = 1.f;
        if (valid[g]) {
            const char *row = Xb + (size_t)id[g] * row_bytes;
            va[g] = *reinterpret_cast<const u32x4_a8 *>(row + 16 * m);
            vb[g] = *reinterpret_cast<const u32x4_a8 *>(row + 256 + 16 * m);
            if (m == 15) nrm[g] = norms ? norms[id[g]] : *reinterpret_cast<const float *>(row + 512);
        }
    }
#pragma unroll
    for (int g = 0; g < G; g++) {
        float sa = feat8_partial_pair(qa, va[g]), sb = feat8_partial_pair(qb, vb[g]);
        sa = dpp_pair_add<0xB1, 0xf>(sa);  // level 2: lane ^ 1
        sb = dpp_pair_add<0xB1, 0xf>(sb);
        sa = dpp_pair_add<0x4E, 0xf>(sa);  // level 3: lane ^ 2
        sb = dpp_pair_add<0x4E, 0xf>(sb);
        sa = dpp_pair_add<0x114, 0xf>(sa); // level 4: row_shr:4
        sb = dpp_pair_add<0x114, 0xf>(sb);
        sa = dpp_pair_add<0x118, 0xf>(sa); // level 5: row_shr:8 -> lanes 12..15 of the row: partials 0..31 / 32..63
        sb = dpp_pair_add<0x118, 0xf>(sb);
        out[g] = 1.0f - (sa + sb) / nrm[g]; // level 6
    }
}

// neighbour list of `node` on level lv: level 0 lists are [n x M0], upper lists [n_upper_lists x M] at upper_off[node] + lv - 1
__device__ __forceinline__ const uint32_t *adj_list(const uint32_t *__restrict__ base, const uint32_t *__restrict__ upper_off, uint32_t deg,
                                                    int lv, uint32_t node) {
    const size_t list = lv == 0 ? (size_t)node : (size_t)upper_off[node] + (uint32_t)(lv - 1);
    return base + list * deg;
}

// LDS carve-up (dynamic): [W0 | W1 | s_key x2 | s_new x2 | misc | (filtered: R0 | R1 | s_keyR x2) | table]
// s_key / s_new / s_keyR exist once per hop parity: wave 0 prepares hop h + 1 (adjacency list through the visited table) while the
// other waves still merge hop h.
struct SearchLds {
    uint64_t *s_key;
    uint32_t *s_new;
    uint32_t *misc;  // [1],[2]=next selection (by hop parity) [3]=table full [4]=pool slot [5]=generation
                     // [6]=1 if the target level's seed is allowed (filtered) [8],[9]=n_new (by hop parity)
                     // [10]=rows the workgroup's waves ruled out on their hi plane (SCREEN); [7], [11]..[15] free
};
// (its size: search_lds_bytes, search_plan.h)

// G16 (recompute-on rows of 256 features only): phase C evaluates four rows per wave instruction (group_dist_rows_feat256), R = groups
// in flight per wave.
// LW: adjacency-list ids per lane of wave 0 — 1 for lists of <= 64 ids, 2 for wide graphs (<= 128 ids: lane l holds ids l and 64 + l).
// Phase B compacts the second half behind the first with a second ballot (the unseen ids keep list order), phase E reduces over both
// keys of a lane and adds a second rank count; phases C and D already loop over n_new.  LW = 1 compiles to the narrow code unchanged.
// SCREEN (throughput form of the plain f32 search only): phase C goes through the split planes (wave_dist_rows_screen; T = 3: its wide form).
// BF16 (search_bf16.hip): the rows are bf16 (g.X names them, g.row_bytes apart); phase C and the entry go through wave_dist_rows_bf16.
// I8 (search_i8.hip): the rows are int8 codes (g.X, g.row_bytes apart) and g.norms names the column scales 2^-e_j [g.ld], which the
// query staging multiplies into the query; phase C and the entry go through wave_dist_rows_i8.
template <int T, int R, int NW, bool FEAT, bool FILT = false, bool G16 = false, int LW = 1, bool SCREEN = false, bool BF16 = false, bool I8 = false>
__device__ void beam_search_one(const GraphView &g, const SearchArgs &a, uint32_t qi, unsigned char *smem) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const auto *const za = lazy_search_args(); // arguments of the rare paths and of the epilogue: read where they are used
    const uint32_t ef = a.ef;
    static_assert(LW == 1 || LW == 2, "lists of at most 128 ids");
    static_assert(!SCREEN || (NW == 4 && !FEAT && !FILT && !G16 && LW == 1), "the row screen exists in the plain throughput form only");
    static_assert(!BF16 || (!FEAT && !G16 && !SCREEN), "bf16 rows: stored vectors, whole rows");
    static_assert(!I8 || (!FEAT && !G16 && !SCREEN && !BF16), "int8 rows: stored vectors, whole rows");
    const uint32_t maxdeg = g.M0 > g.M ? g.M0 : g.M;
    const uint32_t efp = (ef + 1) & ~1u;
    SearchLds s;
    uint64_t *const W0 = reinterpret_cast<uint64_t *>(smem); // buffer b lives at W0 + b*efp (no pointer array: stays out of scratch)
    constexpr uint32_t NBUF = NW > 4 ? 2u : 1u; // latency form of the hop loop: per-parity buffers (search_lds_bytes)
    const uint32_t kstride = maxdeg + 8;
    s.s_key = W0 + 2 * efp;
    s.s_new = reinterpret_cast<uint32_t *>(s.s_key + NBUF * kstride);
    s.misc = s.s_new + NBUF * maxdeg;
    size_t off = 2 * (size_t)efp * 8 + NBUF * ((size_t)maxdeg + 8) * 8 + NBUF * (size_t)maxdeg * 4 + 64;
    off = (off + 15) & ~(size_t)15;
    // filtered: R list (k best allowed keys so far, double buffered) + the new keys with disallowed ones blanked
    const uint32_t kf = FILT ? a.k : 0u, kfp = (kf + 1) & ~1u;
    uint64_t *const R0 = reinterpret_cast<uint64_t *>(smem + off);
    uint64_t *const s_keyR = R0 + 2 * kfp;
    const uint8_t *const allow = FILT ? a.allow + (size_t)qi * a.allow_stride : nullptr;
    uint32_t rsize = 0;
    int rcur = 0;
    if (FILT) off += 2 * (size_t)kfp * 8 + NBUF * ((size_t)maxdeg + 8) * 8;
    uint32_t *table = reinterpret_cast<uint32_t *>(smem + off);
    const uint32_t hbits = a.hash_bits, hsize = 1u << hbits;
    uint32_t vis_limit = hsize - (hsize >> 2); // 75 % load
    uint32_t hbm = 0;                 // 0: visited set in LDS; 1 / 2: in a pool-1 / pool-2 table in HBM (after an overflow)
    unsigned long long *gtab = nullptr;
    uint32_t gslot = 0, gen = 0, gbits = 0;

    // ---- query into registers -----------------------------------------------------------------
    float4 q[T];
    float qa[8], qb[8]; // G16: elements 8m..8m+7 and 128+8m..+7 of the query, m = lane within the DPP row
    {
        const float *qv;
        uint32_t dq = FEAT ? g.feat_h : g.d;
        if (!FEAT && a.q_rows) qv = g.X + (size_t)a.q_rows[qi] * g.ld;
        else qv = a.queries + (size_t)qi * a.ldq;
#pragma unroll
        for (int t = 0; t < T; t++)
            if (!G16) q[t] = vec_load4_guard(qv, dq, t, lane);
        if constexpr (I8) { // q'_j = q_j 2^-e_j: exact (a query element below 2^-90 in magnitude: out of scope, leann_backend.h)
#pragma unroll
            for (int t = 0; t < T; t++) {
                const uint32_t j = 256u * t + 4u * lane;
                if (j < g.ld) { // g.ld is a multiple of 4; the scales of padding columns are 1
                    const float4 sc = *reinterpret_cast<const float4 *>(g.norms + j);
                    q[t].x *= sc.x; q[t].y *= sc.y; q[t].z *= sc.z; q[t].w *= sc.w;
                }
            }
        }
        if (G16) {
#pragma unroll
            for (int i = 0; i < 8; i++) {
                qa[i] = qv[8 * (lane & 15) + i];
                qb[i] = qv[128 + 8 * (lane & 15) + i];
            }
        }
    }

    float rs_E = 0.f;         // SCREEN: the bound's absolute term (row_screen.h (5))
    uint32_t rs_ruled = 0;    // SCREEN: rows this wave ruled out on their hi plane
    if constexpr (SCREEN) {
        float4 qs = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int t = 0; t < T; t++) { qs.x += fabsf(q[t].x); qs.y += fabsf(q[t].y); qs.z += fabsf(q[t].z); qs.w += fabsf(q[t].w); }
        rs_E = rs_abs_term(wave_tree_sum(lane4_sum(qs)));
        if (tid == 0) s.misc[10] = 0; // summed over the waves at exit (the level loop's barriers come before)
    }
    const uint32_t *const adj0_p = g.adj0, *const adjU_p = g.adjU, *const upoff_p = g.upper_off;
    uint32_t n_evals = 1, hops0 = 0, hopsU = 0; // meaningful in wave 0 / lane 0 only
    uint32_t n_vis = 0;
    uint64_t best;
    {
        uint32_t ids[1] = {g.entry};
        float dd[1];
        if (G16) {
            const bool valid[1] = {lane < 16};
            group_dist_rows_feat256<1>(qa, qb, reinterpret_cast<const char *>(g.X), g.row_bytes, ids, valid, lane, dd, g.norms);
            dd[0] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dd[0]), 15));
        } else if (FEAT) wave_dist_rows_feat<T, 1>(q, reinterpret_cast<const char *>(g.X), g.row_bytes, g.feat_h, ids, 1, lane, dd, g.norms);
        else if constexpr (BF16) wave_dist_rows_bf16<T, 1>(q, reinterpret_cast<const uint16_t *>(g.X), g.row_bytes >> 1, ids, 1, lane, dd);
        else if constexpr (I8) wave_dist_rows_i8<T, 1>(q, reinterpret_cast<const int8_t *>(g.X), g.row_bytes, ids, 1, lane, dd);
        else wave_dist_rows<T, 1>(q, g.X, g.ld, ids, 1, lane, dd);
        best = make_key(dd[0], g.entry); // every wave computes the same value
    }

#ifdef LEANN_STAMPS
    uint64_t stamp[8] = {0, 0, 0, 0, 0, 0, 0, 0}; // [7]: hops whose next candidate came from the OLD beam (not from the hop's new keys)
#endif
    uint32_t wsize = 0, level_hops = 0;
    int cur = 0;
    bool aborted = false;
    for (int lv = (int)g.max_level; lv >= (int)a.target_level; --lv) {
        const uint32_t ef_l = (lv == (int)a.target_level) ? ef : 1u;
        const uint32_t deg = lv == 0 ? g.M0 : g.M;
        if (!hbm)
            for (uint32_t i = tid; i < hsize; i += NW * 64) table[i] = LEANN_EMPTY;
        __syncthreads();
        if (tid == 0) {
            W0[0] = best;
            if (hbm) {
                gen = atomicAdd(&za->gpool_ctr[1], 1u) + 1u;
                s.misc[5] = gen;
                vis_insert_hbm(gtab, gbits, gen, key_id(best));
            } else {
                table[vis_hash(key_id(best), hbits)] = key_id(best);
            }
            s.misc[1] = LEANN_EMPTY;
            s.misc[2] = LEANN_EMPTY;
            s.misc[3] = 0;
            if (FILT && lv == (int)a.target_level) {
                const uint32_t e = key_id(best);
                const uint32_t ok = (allow[e >> 3] >> (e & 7)) & 1u;
                if (ok) R0[0] = best;
                s.misc[6] = ok;
            }
        }
        __syncthreads();
        if (hbm) gen = uni(s.misc[5]);
        const bool filt_level = FILT && lv == (int)a.target_level;
        if (filt_level) { rsize = uni(s.misc[6]); rcur = 0; }
        cur = 0;
        wsize = 1;
        n_vis = 1;
        uint32_t sel = 0;
        uint32_t hop = 0;
        // Two forms of the hop loop (identical results: exactly one candidate is expanded per step, in the sequential order).
        // Throughput form (4 waves per query, every CU full): phase B — the adjacency list through the visited table, wave 0 — at the
        // head of the hop, three barriers; its list was prefetched by phase E of the hop before.  Latency form (16 waves per query,
        // batches <= 512): wave 0 runs phase B of hop h + 1 right behind phase E, UNDER the merge of hop h — two barriers per hop, single
        // query 0.365 -> 0.32 ms.  With the chip saturated the adjacency round trip outlasts the merge either way and the leaner wave 0
        // of the throughput form is faster (recompute-on search: 3.05 against 2.98 M queries/s; hnsw10m equal; scripts/exp/ab.sh).
        // Every phase is stated once, in a fragment file included by both forms (hop_adj.cuh B, hop_migrate.cuh the table migration,
        // hop_rows.cuh C, hop_select.cuh E, hop_merge.cuh D, hop_rmerge.cuh the filtered R list): what remains here, and all the two forms
        // differ in, is where phase B sits, the parity of its buffers, the barriers, and the row screen (throughput form only).
        constexpr bool EARLY_B = NW > 4;
        if constexpr (!EARLY_B) {
            // Adjacency list of the NEXT node to expand, LW neighbour ids per lane of wave 0 (lists hold at most 64 LW ids).  The load is
            // issued as soon as the next candidate is known — right after the new distances exist, BEFORE the merge (phase E below) —
            // so its HBM round trip runs under the merge and the barrier instead of at the head of the next hop.
            uint32_t e_pref = LEANN_EMPTY, e_pref1 = LEANN_EMPTY; // e_pref1: ids 64..127 (LW = 2)
            // (level-dependent pieces of the list address as VALUES: selecting between the two struct members by address makes hipcc keep
            // the by-value GraphView in scratch memory)
            const uint32_t *const adj_base = lv == 0 ? adj0_p : adjU_p;
            if (wave == 0) {
                e_pref = (uint32_t)lane < deg ? adj_list(adj_base, upoff_p, deg, lv, key_id(best))[lane] : LEANN_EMPTY;
                if constexpr (LW == 2) e_pref1 = (uint32_t)lane + 64u < deg ? adj_list(adj_base, upoff_p, deg, lv, key_id(best))[lane + 64] : LEANN_EMPTY;
            }
            while (sel != LEANN_EMPTY) {
                uint64_t *Wc = W0 + cur * efp, *Wn = W0 + (cur ^ 1) * efp;
    #ifdef LEANN_STAMPS // diagnostic build only (scripts/stamps.sh): where does a hop spend its cycles?
                const uint64_t st0 = __builtin_amdgcn_s_memtime();
    #endif
                // ---- phase B: adjacency list through the visited table (wave 0) ------------------
                if (wave == 0) {
                    constexpr uint32_t p = 0;
                    const uint64_t ckey = Wc[sel];
                    const uint32_t hidx = hop;
                    #include "hop_adj.cuh"
                }
    #ifdef LEANN_STAMPS
                const uint64_t stB = __builtin_amdgcn_s_memtime();
    #endif
                __syncthreads(); // B1
    #ifdef LEANN_STAMPS
                const uint64_t stB1 = __builtin_amdgcn_s_memtime();
    #endif
                const uint32_t table_full = uni(s.misc[3]);
                if (table_full) {
                    // Table full: move the visited set one level up (LDS -> pool 1 -> pool 2) and redo this hop.
                    #include "hop_migrate.cuh"
                    continue;
                }
                const uint32_t n_new = uni(s.misc[0]);
                uint64_t *const skey = s.s_key, *const skeyR = s_keyR; // the names the shared phases (hop_*.cuh) use;
                const uint32_t *const snew = s.s_new;                  // the latency form has one of each per parity
                // ---- phase C: stream the new rows, R in flight per wave ------------------------------
                if constexpr (SCREEN) {
                    const bool armed = wsize == ef_l; // a full beam: its last entry is the distance to beat
                    const float worst = orderable_f32(uni((uint32_t)(Wc[wsize - 1] >> 32)));
                    if constexpr (T == 3) {
                        // Wide form: one hi-plane round over H rows per wave, then the survivors as whole rows, R at a time.  A beam
                        // that is not full rules nothing out, so its rows skip the hi round: one round trip per R rows.
                        constexpr int H = LEANN_SCREEN_H3;
                        static_assert(H >= 1 && H <= 16, "rows per wave in the hi round");
                        const uint32_t w = uni((uint32_t)wave);
                        for (uint32_t j0 = w; j0 < n_new; j0 += NW * H) {
                            const uint32_t have = min((n_new - j0 + NW - 1) / NW, (uint32_t)H); // rows of this wave in this round
                            uint32_t surv = (1u << have) - 1u;
                            if (armed) {
                                surv = wave_screen_hi_rows<T, H, NW>(q, za->x_hi, za->ldp, s.s_new, s.s_key, j0, n_new, lane, worst, rs_E);
                                rs_ruled += have - (uint32_t)__popc(surv);
                            }
                            wave_dist_rows_planes<T, R, NW>(q, za->x_hi, za->x_lo, za->ldp, s.s_new, s.s_key, j0, surv, lane);
                        }
                    } else
                    for (uint32_t j0 = wave; j0 < n_new; j0 += NW * R) {
                        uint32_t ids[R];
                        float dd[R];
                        int nrows = 0;
    #pragma unroll
                        for (int r = 0; r < R; r++) {
                            uint32_t j = j0 + r * NW;
                            if (j < n_new) { ids[r] = s.s_new[j]; nrows = r + 1; }
                        }
                        const uint32_t ruled = wave_dist_rows_screen<T, R>(q, za->x_hi, za->x_lo, za->ldp, ids, nrows, lane, armed, worst, rs_E, dd);
                        rs_ruled += (uint32_t)__popc(ruled);
                        if (lane == 0) {
    #pragma unroll
                            for (int r = 0; r < R; r++)
                                if (r < nrows) s.s_key[j0 + r * NW] = make_key(dd[r], ids[r]);
                        }
                    }
                } else {
                    #include "hop_rows.cuh"
                }
    #ifdef LEANN_STAMPS
                const uint64_t stC = __builtin_amdgcn_s_memtime();
    #endif
                __syncthreads(); // B2
    #ifdef LEANN_STAMPS
                const uint64_t stB2 = __builtin_amdgcn_s_memtime();
    #endif
                uint32_t *next_slot = &s.misc[1 + (hop & 1)];
                const uint32_t n_pad = (n_new + 7) & ~7u;
                if (wave == 0) {
                    // ---- phase E: the next candidate, known before the merge; its adjacency load is issued now ----------------
                    #include "hop_select.cuh"
                } else {
                    #include "hop_merge.cuh"
                }
                if (filt_level) {
                    #include "hop_rmerge.cuh"
                }
    #ifdef LEANN_STAMPS
                const uint64_t stD = __builtin_amdgcn_s_memtime();
    #endif
                __syncthreads(); // B3
    #ifdef LEANN_STAMPS
                {
                    const uint64_t stE = __builtin_amdgcn_s_memtime();
                    stamp[0] += stB - st0; stamp[1] += stB1 - stB; stamp[2] += stC - stB1; stamp[3] += stB2 - stC;
                    stamp[4] += stD - stB2; stamp[5] += stE - stD; stamp[6] += 1;
                }
    #endif
                sel = uni(*next_slot);
                wsize = min(wsize + n_new, ef_l);
                cur ^= 1;
                hop++;
            }
        } else {
            // Per hop, two workgroup barriers:
            //   C  every wave: distances of the hop's unseen neighbours (rows in flight, wave-tree reductions)            | barrier
            //   E  wave 0: the NEXT candidate, known before the merge — the merged beam's first unexpanded entry is the smaller of the old
            //      beam's first unexpanded entry other than the one just expanded and the smallest new key; its index is the number of
            //      keys below it — then that node's adjacency list (LW ids per lane, lists hold <= 64 LW) through the visited table:
            //      phase B of the next hop, into the other parity's buffers
            //   D  waves 1 .. NW-1, meanwhile: merge by rank into the other beam buffer                                    | barrier
            // The adjacency round trip of hop h + 1 thus runs under the merge of hop h.  Exactly one candidate is expanded per step, in
            // the sequential order: same entry, same index as a scan of the merged list would give.
            const uint32_t *const adj_base = lv == 0 ? adj0_p : adjU_p; // (as VALUES: an address-select between struct members puts the by-value GraphView in scratch)
            uint32_t e_pref = LEANN_EMPTY, e_pref1 = LEANN_EMPTY; // e_pref1: ids 64..127 (LW = 2)
            auto phase_b = [&](uint32_t p, uint64_t ckey, uint32_t hidx) __attribute__((always_inline)) { // wave 0
                #include "hop_adj.cuh"
            };
            if (wave == 0) {
                e_pref = (uint32_t)lane < deg ? adj_list(adj_base, upoff_p, deg, lv, key_id(best))[lane] : LEANN_EMPTY;
                if constexpr (LW == 2) e_pref1 = (uint32_t)lane + 64u < deg ? adj_list(adj_base, upoff_p, deg, lv, key_id(best))[lane + 64] : LEANN_EMPTY;
                phase_b(0u, best, 0u);
            }
            __syncthreads();
            uint32_t par = 0;
            for (;;) {
                uint64_t *Wc = W0 + cur * efp, *Wn = W0 + (cur ^ 1) * efp;
#ifdef LEANN_STAMPS // diagnostic build only (scripts/stamps.sh): where does a hop spend its cycles?
                const uint64_t st0 = __builtin_amdgcn_s_memtime();
#endif
                if (uni(s.misc[3])) {
                    // Table full: move the visited set one level up (LDS -> pool 1 -> pool 2), then wave 0 prepares this hop again.
                    #include "hop_migrate.cuh"
                    if (wave == 0) phase_b(par, Wc[sel], hop);
                    __syncthreads();
                    continue;
                }
                const uint32_t n_new = uni(s.misc[8 + par]);
                uint64_t *const skey = s.s_key + par * kstride;
                const uint32_t *const snew = s.s_new + par * maxdeg;
                uint64_t *const skeyR = s_keyR + par * kstride;
                // ---- phase C: stream the new rows, R in flight per wave ------------------------------
                #include "hop_rows.cuh"
#ifdef LEANN_STAMPS
                const uint64_t stC = __builtin_amdgcn_s_memtime();
#endif
                __syncthreads(); // B2
#ifdef LEANN_STAMPS
                const uint64_t stB2 = __builtin_amdgcn_s_memtime();
#endif
                uint32_t *next_slot = &s.misc[1 + (hop & 1)];
                const uint32_t n_pad = (n_new + 7) & ~7u;
                if (wave == 0) {
                    // ---- phase E: next candidate; then phase B of the next hop ---------------------------------------------
                    #include "hop_select.cuh"
                    if (next != LEANN_EMPTY) phase_b(par ^ 1u, ckey, hop + 1); // waits for the list while the other waves merge
                } else {
                    #include "hop_merge.cuh"
                }
                if (filt_level) {
                    #include "hop_rmerge.cuh"
                }
#ifdef LEANN_STAMPS
                const uint64_t stD = __builtin_amdgcn_s_memtime();
#endif
                __syncthreads(); // B3: the merged beam and the next hop's unseen neighbours are in place
#ifdef LEANN_STAMPS
                {
                    const uint64_t stE = __builtin_amdgcn_s_memtime();
                    stamp[0] += 0; stamp[1] += 0; stamp[2] += stC - st0; stamp[3] += stB2 - stC;
                    stamp[4] += stD - stB2; stamp[5] += stE - stD; stamp[6] += 1;
                }
#endif
                sel = uni(*next_slot);
                wsize = min(wsize + n_new, ef_l);
                cur ^= 1;
                hop++;
                par ^= 1u;
                if (sel == LEANN_EMPTY) break;
            }
        }
        level_hops = hop;
        if (aborted) break;
        best = W0[cur * efp] & ~1ull;
        __syncthreads(); // everyone has read `best` before the next level rewrites W[0]
    }

    // ---- results ------------------------------------------------------------------------------
    __syncthreads();
    if (hbm && tid == 0) atomicExch(&(hbm == 1 ? za->gpool_lock : za->gpool2_lock)[gslot], 0u); // every probe of this workgroup has returned
    if constexpr (SCREEN) { // the handle's running totals: rows ruled out / rows read in full (every evaluation but the entry's)
        if (lane == 0 && rs_ruled) atomicAdd(&s.misc[10], rs_ruled);
        __syncthreads();
        if (tid == 0) {
            const uint32_t ruled = s.misc[10];
            atomicAdd(&za->screen_ctr[0], (unsigned long long)ruled);
            atomicAdd(&za->screen_ctr[1], (unsigned long long)(n_evals - 1u - ruled));
        }
    }
    if (aborted) { // defensive (see the pool comment): the last table level filled up; empty result + stat 3 -> LEANN_ERR_OVERFLOW
        for (uint32_t t = tid; t < za->k; t += NW * 64) {
            za->out_keys[(size_t)qi * za->k + t] = 0xFFFFFFFFFFFFFFFFull;
            za->out_dists[(size_t)qi * za->k + t] = __uint_as_float(0x7F800000u);
        }
        if (tid == 0) {
            za->out_counts[qi] = 0;
            if (za->out_stats) {
                za->out_stats[(size_t)qi * 4 + 0] = n_evals;
                za->out_stats[(size_t)qi * 4 + 1] = hops0;
                za->out_stats[(size_t)qi * 4 + 2] = hopsU;
                za->out_stats[(size_t)qi * 4 + 3] = 3u;
            }
        }
        return;
    }
    const uint32_t nout = FILT ? rsize : min(wsize, za->k);
    uint64_t *Wc = FILT ? R0 + rcur * kfp : W0 + cur * efp;
    for (uint32_t t = tid; t < za->k; t += NW * 64) {
        size_t o = (size_t)qi * za->k + t;
        if (t < nout) {
            uint64_t k = Wc[t];
            za->out_keys[o] = (uint64_t)key_id(k) + za->key_offset;
            za->out_dists[o] = key_dist(k);
        } else {
            za->out_keys[o] = 0xFFFFFFFFFFFFFFFFull;
            za->out_dists[o] = __uint_as_float(0x7F800000u);
        }
    }
#ifdef LEANN_STAMPS
    if (tid == 0 && za->out_expanded == nullptr && za->exp_cap == 0xFEED) { // stamps go to a buffer of their own (passed via out_nexp)
        unsigned long long *dst = reinterpret_cast<unsigned long long *>(za->out_nexp) + (size_t)qi * 8;
        for (int i = 0; i < 8; i++) dst[i] = stamp[i];
    }
#endif
    if (tid == 0) {
        za->out_counts[qi] = nout;
        if (za->out_nexp && za->exp_cap != 0xFEED) za->out_nexp[qi] = min(level_hops, za->exp_cap);
        if (za->out_stats) {
            za->out_stats[(size_t)qi * 4 + 0] = n_evals;
            za->out_stats[(size_t)qi * 4 + 1] = hops0;
            za->out_stats[(size_t)qi * 4 + 2] = hopsU;
            za->out_stats[(size_t)qi * 4 + 3] = hbm; // 0 LDS table only, 1 / 2 the visited set moved to pool 1 / 2
        }
    }
    __syncthreads();
}

// One workgroup per query.  BUILD only names the instantiation used by index construction (queries are
// base rows, k = ef) so that profiles keep query launches and construction launches apart.
// Narrow rows (<= 512 floats) are short of workgroups per CU, not of HBM (api.hip gives them the 16 KiB visited table): the compiler is
// asked for 6 workgroups per CU at 257..512 floats (80 registers instead of 83, no spill; 384-d 1.84 -> 1.95 M queries/s) and for 8 at
// <= 256 floats (64 registers, one spilled; 128-d 3.10 -> 3.64 M, 256-d 2.67 -> 2.80 M; scripts/exp/dims_sweep.py through scripts/variant.sh).
#ifndef LEANN_T2_OCC
#define LEANN_T2_OCC 6
#endif
#ifndef LEANN_T1_OCC
#define LEANN_T1_OCC 8
#endif
template <int T, int R, int NW, bool BUILD>
__global__ void __launch_bounds__(NW * 64, (NW == 4 && T == 2) ? LEANN_T2_OCC : (NW == 4 && T == 1) ? LEANN_T1_OCC : 1) beam_search_kernel(GraphView g, SearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t qi = blockIdx.x;
    if (qi >= a.nq) return;
    beam_search_one<T, R, NW, false>(g, a, qi, smem);
}
// Throughput form (4 waves per query) of the plain search with the split-plane row screen; api.hip launches it only for a handle
// whose planes are in place (T = 3 and 6: 768-d and 1 536-d rows).
// Workgroups per CU the compiler is asked to leave registers for: the hi and lo halves of R rows (T = 3: the hi halves of
// LEANN_SCREEN_H3 rows, then both halves of R), the query and two sets of accumulators are live together.
#ifndef LEANN_SCREEN_OCC3
#define LEANN_SCREEN_OCC3 4
#endif
#ifndef LEANN_SCREEN_OCC6
#define LEANN_SCREEN_OCC6 3
#endif
template <int T, int R>
__global__ void __launch_bounds__(256, T == 3 ? LEANN_SCREEN_OCC3 : LEANN_SCREEN_OCC6) beam_search_screen_kernel(GraphView g, SearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t qi = blockIdx.x;
    if (qi >= a.nq) return;
    beam_search_one<T, R, 4, false, false, false, 1, true>(g, a, qi, smem);
}
// filtered search (allow-bitmap): answers come from the R list
template <int T, int R, int NW>
__global__ void __launch_bounds__(NW * 64) beam_search_filtered_kernel(GraphView g, SearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t qi = blockIdx.x;
    if (qi >= a.nq) return;
    beam_search_one<T, R, NW, false, true>(g, a, qi, smem);
}
template <int T, int R, int NW>
__global__ void __launch_bounds__(NW * 64) beam_search_feat_filtered_kernel(GraphView g, SearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t qi = blockIdx.x;
    if (qi >= a.nq) return;
    beam_search_one<T, R, NW, true, true>(g, a, qi, smem);
}
// Throughput instantiation of the recompute-on search (4 waves per query, 520-B rows): the memory system delivers random 520-B rows at
// no more than ~3.9 TB/s however many are in flight (scripts/micro/gather_bw.hip: 4.8 TB/s of 128-B lines; 3 KiB rows reach 6.4), and the
// kernel gets closest to that with MANY queries per CU rather than many rows per wave: 8 workgroups per CU (the 16 KiB visited tables
// allow 8) at 5 rows in flight per wave — a typical hop has ~24 unseen neighbours = 6 per wave — measured 3.14 M queries/s against 2.91 M
// at 6 workgroups x 8 rows and 3.08 M at 7 x 6 (recompute10m_graph, ef = 56; scripts/exp/feat_occupancy.sh).
#ifndef LEANN_FEAT_OCC
#define LEANN_FEAT_OCC 8
#endif
// recompute-on rows of exactly 256 features: four rows per wave instruction, G groups in flight per wave (G16 above).  Throughput
// shape = 7 workgroups per CU x 1 group (72 registers, no spills; 16 rows per workgroup and round): 4.5 M queries/s at ef = 52 =
// 7.9 G random rows/s, against the 10 G rows/s scripts/micro/gather_bw.hip measures as the memory system's ceiling for this access
// shape.  6 workgroups x 2 groups (a typical hop's ~26 unseen neighbours in ONE round) is 2 % behind, 8 workgroups (64 registers) spill:
// 3.7-3.9 M, 6 x 3 groups 3.5 M (scripts/exp/feat256_shape.sh).
#ifndef LEANN_FEAT256_OCC
#define LEANN_FEAT256_OCC 7
#endif
template <int G, int NW>
__global__ void __launch_bounds__(NW * 64, NW == 4 ? LEANN_FEAT256_OCC : 1) beam_search_feat256_kernel(GraphView g, SearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t qi = blockIdx.x;
    if (qi >= a.nq) return;
    beam_search_one<1, G, NW, true, false, true>(g, a, qi, smem);
}
template <int G, int NW>
__global__ void __launch_bounds__(NW * 64) beam_search_feat256_filtered_kernel(GraphView g, SearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t qi = blockIdx.x;
    if (qi >= a.nq) return;
    beam_search_one<1, G, NW, true, true, true>(g, a, qi, smem);
}
// recompute-on instantiation: rows are bf16 features + inline norm, queries are W q
template <int T, int R, int NW>
__global__ void __launch_bounds__(NW * 64, (NW == 4 && T == 1) ? LEANN_FEAT_OCC : 1) beam_search_feat_kernel(GraphView g, SearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t qi = blockIdx.x;
    if (qi >= a.nq) return;
    beam_search_one<T, R, NW, true>(g, a, qi, smem);
}

// Wide graphs (M0 or M > 64, lists of up to 128 ids: HNSW M <= 64, DiskANN R <= 128): the same kernels with two list ids per lane of
// wave 0 (LW = 2 above).  Separate templates, so the narrow kernels keep their symbols and code objects; api.hip dispatches here only
// when max(M, M0) > 64.  No occupancy requests: wide lists double a hop's unseen neighbours and the tuning above was measured on
// narrow graphs.
template <int T, int R, int NW, bool BUILD>
__global__ void __launch_bounds__(NW * 64) wide_beam_search_kernel(GraphView g, SearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t qi = blockIdx.x;
    if (qi >= a.nq) return;
    beam_search_one<T, R, NW, false, false, false, 2>(g, a, qi, smem);
}
template <int T, int R, int NW>
__global__ void __launch_bounds__(NW * 64) wide_beam_search_filtered_kernel(GraphView g, SearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t qi = blockIdx.x;
    if (qi >= a.nq) return;
    beam_search_one<T, R, NW, false, true, false, 2>(g, a, qi, smem);
}
template <int T, int R, int NW>
__global__ void __launch_bounds__(NW * 64) wide_beam_search_feat_kernel(GraphView g, SearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t qi = blockIdx.x;
    if (qi >= a.nq) return;
    beam_search_one<T, R, NW, true, false, false, 2>(g, a, qi, smem);
}
template <int T, int R, int NW>
__global__ void __launch_bounds__(NW * 64) wide_beam_search_feat_filtered_kernel(GraphView g, SearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t qi = blockIdx.x;
    if (qi >= a.nq) return;
    beam_search_one<T, R, NW, true, true, false, 2>(g, a, qi, smem);
}
template <int G, int NW>
__global__ void __launch_bounds__(NW * 64) wide_beam_search_feat256_kernel(GraphView g, SearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t qi = blockIdx.x;
    if (qi >= a.nq) return;
    beam_search_one<1, G, NW, true, false, true, 2>(g, a, qi, smem);
}
template <int G, int NW>
__global__ void __launch_bounds__(NW * 64) wide_beam_search_feat256_filtered_kernel(GraphView g, SearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t qi = blockIdx.x;
    if (qi >= a.nq) return;
    beam_search_one<1, G, NW, true, true, true, 2>(g, a, qi, smem);
}
