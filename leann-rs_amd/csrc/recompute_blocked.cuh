// recompute_blocked.cuh — the general encode kernel for dims > 768 (included by recompute.hip only).
// encode_kernel<CT, ..> keeps a 128-passage x ALL-columns tile in accumulators (192 registers at CT = 6) and a 3-slot ring of
// all-column k-step slabs in LDS (159 of 160 KiB at dp = 768, h = 256): neither fits twice.  encode_blocked_kernel<FUSED, POOL>
// keeps the feature tile sF[128][hp + 8] in LDS for the whole workgroup and walks the columns in blocks of CT * 128
// (encode_plan.h: CT in {1, 2, 3, 4, 6}, block b = columns [col0_b, col0_b + CT_b * 128) of every k-step slab of the SAME
// Wp[kstep][dp][16] image).  A block runs the phases of encode_kernel, from the same fragments (encode_ring.cuh, encode_kloop.cuh,
// encode_pool.cuh, encode_score.cuh; encode_features.cuh and encode_mask.cuh once in front of the blocks); what is this kernel's own:
//   * sums of squares: added to sN block after block (SN_ADD), combined after the last block (encode_norm.cuh).
//   * FUSED: the three G pieces ride in the slabs of the LAST block only and the score MFMAs run there (SCORE: the score tile is then
//     live in registers for one block, not for all of them); score = accs / nrm with nrm taken after the last block.
//   * not FUSED: the row norm is known only after the last block, so every thread stores its unnormalised values as its blocks finish
//     and, after the last block, re-reads exactly the addresses it wrote and stores value / nrm (same thread, same addresses:
//     program order, no cross-thread visibility involved).  The GEMM runs once.
#pragma once
#include "encode_plan.h"

struct EncodeBlocks { // column blocks of one launch, by value: 4 bits per block, so that a block's width is scalar shifts of kernel
    uint32_t n;       // arguments (a by-value array indexed at run time would live in scratch memory)
    uint64_t w[2];
    __host__ __device__ uint32_t ctb(uint32_t b) const { return (uint32_t)(w[b >> 4] >> ((b & 15) * 4)) & 15u; }
    void set(uint32_t b, uint32_t c) { w[b >> 4] |= (uint64_t)c << ((b & 15) * 4); }
};
static_assert(LEANN_ENCODE_MAX_BLOCKS <= 32, "EncodeBlocks packs 32 blocks");

template <bool FUSED, bool POOL>
__global__ void __launch_bounds__(512) encode_blocked_kernel(const uint16_t *__restrict__ F, uint64_t n, uint32_t h, uint32_t hp,
                                                             const uint16_t *__restrict__ Wp, uint32_t d, uint32_t dp, uint32_t ld_out,
                                                             float *E, const uint16_t *__restrict__ Gp, uint32_t nq,
                                                             float *__restrict__ S, uint32_t n_rows_s, uint32_t L,
                                                             const uint8_t *__restrict__ mask, float *__restrict__ norms_out,
                                                             const EncodeBlocks blocks) {
    constexpr int RING = 3; // k-step slabs in LDS: one being consumed, two in flight
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t fstride = hp + 8; // bf16 elements per sF row
    uint16_t *sF = reinterpret_cast<uint16_t *>(smem);
    float *sN = reinterpret_cast<float *>(sF + 128 * fstride); // [4 col groups][128 rows] sum of squares over the blocks so far
    float *sM = sN + 4 * 128;                                   // [128] attention mask of the tile's token rows (0/1)
    float *sC = sM + 128;                                       // [128] max(token count, 1e-9) at each passage's first row
    uint16_t *sW = reinterpret_cast<uint16_t *>(sC + 128);      // [RING][block columns (+192)][16] linear, swizzled 16-B slots
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int rhalf = wave >> 2, cgrp = wave & 3;
    const int st = cgrp >> 1, qt = cgrp & 1;
    const uint64_t row_base = (uint64_t)blockIdx.x * 128;
    const uint32_t nks = hp / 16;

#include "encode_features.cuh" // the feature tile -> sF, once: it stays for every column block
    sN[tid] = 0.f; // 512 threads = 4 x 128 entries
#include "encode_mask.cuh" // sM, sC; its barrier publishes the feature tile and the zeroed sN
    // One column block: CT tiles of 32 columns per wave starting at column col0; SCORE = the block that also carries G.
    auto run_block = [&](auto ct_c, auto score_c, const uint32_t col0) __attribute__((always_inline)) {
        constexpr int CT = decltype(ct_c)::value;
        constexpr bool SCORE = decltype(score_c)::value;
        constexpr int DP = CT * 128;                // columns of the block
        constexpr int DPX = DP + (SCORE ? 192 : 0); // + three 64-query pieces of G
        constexpr int NI = DPX * 2 / 64;            // 1-KiB DMA instructions per k-step slab
        constexpr int PER = (NI + 7) / 8;           // ... per wave (the same count in every wave: counted vmcnt waits)
        // The lane's indices are re-derived per block from an opaque copy of the thread id: hipcc otherwise hoists the address
        // arithmetic of all five block widths in front of the block loop and spills ~100 registers of it into the k-loops.
        int tid_b = tid;
        asm volatile("" : "+v"(tid_b));
        const int lane = tid_b & 63, wave = tid_b >> 6, l31 = lane & 31, lh = lane >> 5, rhalf = wave >> 2, cgrp = wave & 3;
        const int st = cgrp >> 1, qt = cgrp & 1;
#include "encode_ring.cuh" // stage_w, frag, acc = 0, accs = 0 (the score tile lives in the last block only)
        // Everybody is past the barrier that closed the previous block's k-loop, so the ring is free; the previous block's
        // stores (not FUSED) are retired first so that the counted waits of the k-loop count DMA instructions only.
        if (!FUSED) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#include "encode_kloop.cuh" // acc = F W over the block's columns, SCORE: accs = G F^T
        __syncthreads(); // every wave is done with the ring (all DMA waited for: a plain barrier)
        constexpr bool SN_ADD = true; // this block's share of the row sums of squares is added to the blocks' before it
#include "encode_pool.cuh" // POOL: acc = masked mean over the L token rows; sN += the block's sums of squares
        // ---- not FUSED: the unnormalised values of the block (normalised in place after the last block) -------
        if (!FUSED) {
#pragma unroll
            for (int rt = 0; rt < 2; rt++) {
#pragma unroll
                for (int reg = 0; reg < 16; reg++) {
                    const int r = rhalf * 64 + rt * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
                    const uint64_t row = row_base + r;
                    if (row < n && (r % L) == 0) {
#pragma unroll
                        for (int ct = 0; ct < CT; ct++) {
                            const uint32_t col = col0 + (cgrp * CT + ct) * 32 + l31;
                            if (col < ld_out) E[(size_t)(row / L) * ld_out + col] = col < d ? acc[rt][ct][reg] : 0.f;
                        }
                    }
                }
            }
        }
        if constexpr (SCORE) { // the last block
            __syncthreads(); // the sums of squares of every block and column group are in sN
#include "encode_score.cuh" // S = accs / nrm
        }
    };

    {
        uint32_t col0 = 0;
        for (int b = 0; b < (int)blocks.n; b++) {
            const int c = (int)blocks.ctb((uint32_t)b);
            const bool score = FUSED && b == (int)blocks.n - 1;
#define LEANN_RUN_BLOCK(C)                                                                            \
    case C:                                                                                           \
        if constexpr (FUSED) {                                                                        \
            if (score) run_block(std::integral_constant<int, C>{}, std::true_type{}, col0);           \
            else run_block(std::integral_constant<int, C>{}, std::false_type{}, col0);                \
        } else run_block(std::integral_constant<int, C>{}, std::false_type{}, col0);                  \
        break;
            switch (c) {
                LEANN_RUN_BLOCK(1)
                LEANN_RUN_BLOCK(2)
                LEANN_RUN_BLOCK(3)
                LEANN_RUN_BLOCK(4)
                LEANN_RUN_BLOCK(6)
                default: break;
            }
#undef LEANN_RUN_BLOCK
            col0 += (uint32_t)c * 128;
        }
    }
    if (FUSED) return; // the last block stored the scores
    __syncthreads(); // the sums of squares of every block and column group are in sN
    // ---- normalise in place: each thread revisits exactly the elements it stored ------------------------------
    for (int rt = 0; rt < 2; rt++) {
        for (int reg = 0; reg < 16; reg++) {
            const int r = rhalf * 64 + rt * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
            const uint64_t row = row_base + r;
#include "encode_norm.cuh" // nrm
            if (!(row < n && (r % L) == 0)) continue;
            if (norms_out && cgrp == 0 && l31 == 0) norms_out[row / L] = nrm; // ||W^T f|| before normalisation
            float *erow = E + (size_t)(row / L) * ld_out;
            uint32_t col0 = 0;
            for (int b = 0; b < (int)blocks.n; b++) {
                const uint32_t c = blocks.ctb((uint32_t)b);
                for (uint32_t ct = 0; ct < c; ct++) {
                    const uint32_t col = col0 + (cgrp * c + ct) * 32 + l31;
                    if (col < ld_out) erow[col] = erow[col] / nrm;
                }
                col0 += c * 128;
            }
        }
    }
}
