// prune.cuh — the select-neighbours heuristic (HNSW Alg. 4 / Vamana RobustPrune) over a candidate pool held in LDS, shared by the
// builder (build.hip) and delete consolidation (consolidate.hip).
#pragma once
#include "common.cuh"

// Candidate pool of one prune: NC = 128 for lists of <= 64 ids; wide graphs (lists of up to 128 ids: HNSW M > 32, DiskANN R > 64)
// take their own instantiations with NC = 256, so that a full 128-id list can still take proposals.  Their lower triangle (127.5 KiB)
// plus the staging tile and the small arrays (~152 KiB of LDS) leave one workgroup per CU; narrow builds keep their kernels.
#define NCMAX 128
#define NCWIDE 256
template <int NC> struct Pool {
    static constexpr int TRI = NC * (NC - 1) / 2;
    static constexpr int KC = 16 * (256 / NC); // gram_lower staging tile: KC x LDW floats; one 16-float piece of a row per thread
    static constexpr int LDW = NC + 4;
    static constexpr int STAGE = NC > NCMAX ? KC * LDW : 1; // wide: a tile of its own (see gram_lower); narrow: inside the triangle
    static constexpr int KS = NC > NCMAX ? 2 : 1;           // kept slots per lane of wave 0 in prune_core
};

// ------------------------------------------------------------------------------------------------
// prune_core: candidates (ids c_id, dists-to-p c_d, ascending by (dist, id)) -> up to `limit` kept.
// alpha == 0: HNSW rule (drop c if dist(c, kept) < dist(c, p)); alpha > 0: Vamana rule
// (drop c if alpha * dist(c, kept) <= dist(c, p)).   256 threads.  Returns count in every thread;
// kept candidate positions in s_sel[0..count).
// ------------------------------------------------------------------------------------------------
template <int TS, int NC = NCMAX> // per-thread tile TS x TS; the (NC/8) x (NC/8) tile grid covers NC/8*TS candidates
__device__ __forceinline__ void gram_lower(const float *__restrict__ X, uint32_t ld, const uint32_t *c_id, uint32_t nc,
                                           float *tri, float *stage_) {
    float *stage = static_cast<float *>(__builtin_assume_aligned(stage_, 16));
    constexpr int KC = Pool<NC>::KC, LDW = Pool<NC>::LDW; // rows of the staging tile stay 16-byte aligned: the 2 x TS operands of a k step are 16-B LDS reads
    constexpr int TD = NC / 8, RS = 256 / NC;              // tile rows / columns; threads per staged row
    // The blocks that touch the lower triangle of the nc x nc matrix — (ty, tx) with tx <= ty < ceil(nc / TS) — are handed to the FIRST
    // threads of the workgroup in triangular order, so the multiply loop runs in ceil(ntiles / 64) waves (1 for the ~70 candidates of a
    // full Vamana list) instead of in every wave that owns a row of a 16 x 16 thread grid (3 of 4 there, a handful of lanes each).
    // Wide pools (NC = 256: up to 528 tiles of 8 x 8) walk the tile list in passes of 256 tiles, each streaming the rows again; their
    // staging tile lives outside the triangle, which the passes before have begun to fill.
    const int tid = threadIdx.x;
    const int tdim = min(TD, (int)((nc + TS - 1) / TS)), ntiles = tdim * (tdim + 1) / 2;
    for (int t0 = 0; t0 < ntiles; t0 += 256) {
    const int tile = t0 + tid;
    const bool active = tile < ntiles;
    int ty = 0, tx = 0;
    if (active) {
        ty = (int)((sqrtf(8.f * (float)tile + 1.f) - 1.f) * 0.5f);
        while (ty * (ty + 1) / 2 > tile) ty--;
        while ((ty + 1) * (ty + 2) / 2 <= tile) ty++;
        tx = tile - ty * (ty + 1) / 2;
    }
    float acc[TS][TS];
#pragma unroll
    for (int i = 0; i < TS; i++)
#pragma unroll
        for (int j = 0; j < TS; j++) acc[i][j] = 0.f;
    const int srow = tid / RS, shalf = tid % RS;
    const float *rowp = (srow < (int)nc) ? X + (size_t)c_id[srow] * ld : nullptr;
    for (uint32_t k0 = 0; k0 < ld; k0 += KC) {
        float4 v[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            uint32_t j = k0 + shalf * 16 + e * 4;
            v[e] = (rowp && j < ld) ? *reinterpret_cast<const float4 *>(rowp + j) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        __syncthreads(); // previous chunk fully consumed
        if (srow < TD * TS) {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                int kk = shalf * 16 + e * 4;
                stage[(kk + 0) * LDW + srow] = v[e].x;
                stage[(kk + 1) * LDW + srow] = v[e].y;
                stage[(kk + 2) * LDW + srow] = v[e].z;
                stage[(kk + 3) * LDW + srow] = v[e].w;
            }
        }
        __syncthreads();
        if (active) {
#pragma unroll 4
            for (int kk = 0; kk < KC; kk++) {
                float a[TS], b[TS];
#pragma unroll
                for (int i = 0; i < TS; i++) a[i] = stage[kk * LDW + ty * TS + i];
#pragma unroll
                for (int j = 0; j < TS; j++) b[j] = stage[kk * LDW + tx * TS + j];
#pragma unroll
                for (int i = 0; i < TS; i++)
#pragma unroll
                    for (int j = 0; j < TS; j++) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
            }
        }
    }
    __syncthreads(); // stage dead; tri may be written
    if (active) {
#pragma unroll
        for (int i = 0; i < TS; i++)
#pragma unroll
            for (int j = 0; j < TS; j++) {
                int r = ty * TS + i, c = tx * TS + j;
                if (c < r && r < (int)nc) tri[r * (r - 1) / 2 + c] = 1.0f - acc[i][j];
            }
    }
    __syncthreads();
    }
}

// NC = NCWIDE: up to 128 kept, two slots per lane (slot s in lane s % 64); `stage` is then a tile of its own (Pool<NC>::STAGE floats).
template <int NC = NCMAX>
__device__ uint32_t prune_core(const float *__restrict__ X, uint32_t ld, const uint32_t *c_id, const float *c_d,
                               uint32_t nc, uint32_t limit, float alpha, float *tri /* Pool<NC>::TRI floats, LDS */,
                               uint32_t *s_sel /* [64 KS] LDS */, uint32_t *s_cnt /* LDS */, bool stage1, float *wide_stage = nullptr) {
    float *stage = static_cast<float *>(__builtin_assume_aligned(NC > NCMAX ? wide_stage : tri, 16)); // narrow: [KC][LDW] aliased, dead before tri is written
    constexpr int KS = Pool<NC>::KS;
    const int tid = threadIdx.x;
    if (nc <= 32) gram_lower<2, NC>(X, ld, c_id, nc, tri, stage);       // work ~ nc^2: small lists use small tiles
    else if (nc <= 64) gram_lower<4, NC>(X, ld, c_id, nc, tri, stage);
    else gram_lower<8, NC>(X, ld, c_id, nc, tri, stage);
    __shared__ uint8_t s_taken[NC];
    if (tid < 64) { // wave 0: sequential walk over candidates, lanes = kept slots
        uint32_t ns = 0;
        int my = -1, my1 = -1; // my1: kept slot 64 + lane (KS = 2)
        // Vamana, two-stage form (DiskANN's occlude_list): the FIRST walk over the whole pool keeps a candidate only if no kept
        // one is at least as close to it as the point itself (alpha = 1: the diverse core, which reaches the far end of the pool before
        // the list is full); only the slots still free after it are filled by the relaxed rule alpha * d(c, kept) <= d(c, p) -> drop.
        // With the one-stage rule of the paper (Alg. 2) at alpha = 1.2 almost nothing is occluded on data of high intrinsic dimension, a
        // list is simply the R nearest of the pool, and at R = 32 the graph stops being navigable as the corpus grows (recall@10 at
        // L = 128, 256-d: 0.976 at 1M, 0.905 at 5M, 0.78 at 10M; scripts/exp/vamana_scale.py, profiles/r03_vamana_scale.md).
        const bool two_stage = alpha > 1.0f && stage1;
        if (two_stage)
            for (uint32_t i = tid; i < nc; i += 64) s_taken[i] = 0;
        for (uint32_t i = 0; i < nc; i++) {
            const float di = c_d[i];
            bool bad = false;
            if (tid < (int)ns) {
                float gdist = tri[i * (i - 1) / 2 + my];
                bad = (alpha == 0.f) ? (gdist < di) : ((two_stage ? 1.0f : alpha) * gdist <= di);
            }
            if (KS == 2 && tid + 64 < (int)ns) {
                float gdist = tri[i * (i - 1) / 2 + my1];
                bad = bad || ((alpha == 0.f) ? (gdist < di) : ((two_stage ? 1.0f : alpha) * gdist <= di));
            }
            if (!__any(bad)) {
                if (tid == (int)ns) my = (int)i;
                if (KS == 2 && tid + 64 == (int)ns) my1 = (int)i;
                if (two_stage && tid == 0) s_taken[i] = 1;
                ns++;
                if (ns == limit) break;
            }
        }
        if (two_stage && ns < limit) {
            for (uint32_t i = 0; i < nc; i++) {
                if (s_taken[i]) continue; // (uniform: every lane reads the same byte)
                const float di = c_d[i];
                bool bad = false;
                if (tid < (int)ns) {
                    const uint32_t hi = max(i, (uint32_t)my), lo = min(i, (uint32_t)my);
                    bad = alpha * tri[hi * (hi - 1) / 2 + lo] <= di;
                }
                if (KS == 2 && tid + 64 < (int)ns) {
                    const uint32_t hi = max(i, (uint32_t)my1), lo = min(i, (uint32_t)my1);
                    bad = bad || alpha * tri[hi * (hi - 1) / 2 + lo] <= di;
                }
                if (!__any(bad)) {
                    if (tid == (int)ns) my = (int)i;
                    if (KS == 2 && tid + 64 == (int)ns) my1 = (int)i;
                    ns++;
                    if (ns == limit) break;
                }
            }
        }
        if (tid < (int)ns) s_sel[tid] = (uint32_t)my;
        if (KS == 2 && tid + 64 < (int)ns) s_sel[tid + 64] = (uint32_t)my1;
        if (tid == 0) *s_cnt = ns;
    }
    __syncthreads();
    return *s_cnt;
}
