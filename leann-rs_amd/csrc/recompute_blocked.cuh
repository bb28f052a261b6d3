// recompute_blocked.cuh — the general encode kernel for dims > 768 (included by recompute.hip only).
// encode_kernel<CT, ..> keeps a 128-passage x ALL-columns tile in accumulators (192 registers at CT = 6) and a 3-slot ring of
// all-column k-step slabs in LDS (159 of 160 KiB at dp = 768, h = 256): neither fits twice.  encode_blocked_kernel<FUSED, POOL>
// keeps the feature tile sF[128][hp + 8] in LDS for the whole workgroup and walks the columns in blocks of CTB * 128
// (encode_plan.h: CTB in {1, 2, 3, 4, 6}, block b = columns [col0_b, col0_b + CTB_b * 128) of every k-step slab of the SAME
// Wp[kstep][dp][16] image), each block running encode_kernel's k-loop: 3-slot LDS-DMA ring, counted vmcnt, one raw barrier per k-step.
//   * sums of squares: per block the narrow kernel's arithmetic (fmaf over the block's tiles, 5-step butterfly over the 32 lanes of a
//     tile), added to sN[column group][row] by the one lane that owns the entry, block after block; the four column groups are
//     combined after the last block as encode_kernel does.  No atomics: the same input gives the same bits.
//   * FUSED: the three G pieces ride in the slabs of the LAST block only and the score MFMAs run there (the score tile is then live in
//     registers for one block, not for all of them); score = accs / nrm with nrm taken after the last block.
//   * not FUSED: the row norm is known only after the last block, so every thread stores its unnormalised values as its blocks finish
//     and, after the last block, re-reads exactly the addresses it wrote and stores value / nrm (same thread, same addresses:
//     program order, no cross-thread visibility involved).  The GEMM runs once.
//   * POOL: masked mean pooling per block in registers before squaring, as in encode_kernel.
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

    // ---- stage the feature tile once (zero-padded rows / k); it stays for every column block ----------------
    for (uint32_t idx = tid; idx < 128 * (hp / 8); idx += 512) {
        const uint32_t r = idx / (hp / 8), k8 = (idx % (hp / 8)) * 8;
        uint4 v = make_uint4(0, 0, 0, 0);
        const uint64_t row = row_base + r;
        if (row < n) {
            if (k8 + 8 <= h && ((h & 7) == 0)) v = *reinterpret_cast<const uint4 *>(F + row * h + k8);
            else {
                uint16_t t[8];
                for (int e = 0; e < 8; e++) t[e] = (k8 + e < h) ? F[row * h + k8 + e] : (uint16_t)0;
                memcpy(&v, t, 16);
            }
        }
        *reinterpret_cast<uint4 *>(sF + r * fstride + k8) = v;
    }
    sN[tid] = 0.f; // 512 threads = 4 x 128 entries
    if (POOL && tid < 128) {
        const uint64_t row = row_base + tid;
        sM[tid] = (row < n && (!mask || mask[row] != 0)) ? 1.f : 0.f;
    }
    __syncthreads(); // feature tile + mask visible (no DMA in flight yet: a plain barrier)
    if (POOL && tid < 128 && (tid % L) == 0) {
        float c = 0.f;
        for (uint32_t j = 0; j < L; j++) c += sM[tid + j];
        sC[tid] = c < 1e-9f ? 1e-9f : c; // candle.rs:213 count.clamp(1e-9, inf)
    }
    auto frag = [](const uint16_t *region, uint32_t col, int lh) -> bf16x8 { // 8 consecutive k of one column (16 B)
        const uint32_t g = 2 * col + lh, p = g ^ ((g >> 4) & 1);
        return *reinterpret_cast<const bf16x8 *>(reinterpret_cast<const char *>(region) + p * 16);
    };
    // One column block: CTB tiles of 32 columns per wave starting at column col0; SCORE = the block that also carries G.
    auto run_block = [&](auto ctb_c, auto score_c, const uint32_t col0) __attribute__((always_inline)) {
        constexpr int CTB = decltype(ctb_c)::value;
        constexpr bool SCORE = decltype(score_c)::value;
        constexpr int DPB = CTB * 128;               // columns of the block
        constexpr int DPX = DPB + (SCORE ? 192 : 0); // + three 64-query pieces of G
        constexpr int NI = DPX * 2 / 64;             // 1-KiB DMA instructions per k-step slab
        constexpr int PER = (NI + 7) / 8;            // ... per wave (the same count in every wave: counted vmcnt waits)
        // The lane's indices are re-derived per block from an opaque copy of the thread id: hipcc otherwise hoists the address
        // arithmetic of all five block widths in front of the block loop and spills ~100 registers of it into the k-loops.
        int tid_b = tid;
        asm volatile("" : "+v"(tid_b));
        const int lane = tid_b & 63, wave = tid_b >> 6, l31 = lane & 31, lh = lane >> 5, rhalf = wave >> 2, cgrp = wave & 3;
        const int st = cgrp >> 1, qt = cgrp & 1;
        // slot p of the block's slab holds piece p ^ ((p >> 4) & 1) of the block's column range (swizzle on the SOURCE address)
        auto stage_w = [&](int slot, uint32_t ks) {
            const char *wsrc = reinterpret_cast<const char *>(Wp + ((size_t)ks * dp + col0) * 16);
            const char *gsrc = SCORE ? reinterpret_cast<const char *>(Gp + (size_t)ks * 192 * 16) : nullptr;
            char *dst = reinterpret_cast<char *>(sW + slot * DPX * 16);
#pragma unroll
            for (int j = 0; j < PER; j++) {
                uint32_t i = wave + 8 * j;
                if (i >= (uint32_t)NI) i = NI - 1; // padding instruction: re-fetches the last piece (same bytes, same place)
                const uint32_t p = i * 64 + lane, g = p ^ ((p >> 4) & 1);
                const char *src = (!SCORE || g < (uint32_t)(DPB * 2)) ? wsrc + (size_t)g * 16 : gsrc + (size_t)(g - DPB * 2) * 16;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                                 (__attribute__((address_space(3))) void *)(dst + i * 1024), 16, 0, 0);
            }
        };
        f32x16 acc[2][CTB];
        f32x16 accs; // SCORE: scores of query tile (cgrp & 1) x passage tile (2*rhalf + (cgrp >> 1)); lives in this block only
#pragma unroll
        for (int i = 0; i < 16; i++) accs[i] = 0.f;
#pragma unroll
        for (int rt = 0; rt < 2; rt++)
#pragma unroll
            for (int ct = 0; ct < CTB; ct++)
#pragma unroll
                for (int i = 0; i < 16; i++) acc[rt][ct][i] = 0.f;
        // Everybody is past the barrier that closed the previous block's k-loop, so the ring is free; the previous block's
        // stores (not FUSED) are retired first so that the counted waits below count DMA instructions only.
        if (!FUSED) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        stage_w(0, 0);
        if (nks > 1) stage_w(1, 1);
        for (uint32_t ks = 0; ks < nks; ks++) {
            // as encode_kernel: (a) my pieces of slab ks have landed, (b) everybody's have and everybody is done reading slab
            // ks-1, so (c) its slot can take slab ks+2
            if (ks + 1 < nks) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (ks + 2 < nks) stage_w((ks + 2) % RING, ks + 2);
            const uint16_t *w = sW + (ks % RING) * DPX * 16;
            bf16x8 a[2], b[CTB];
#pragma unroll
            for (int rt = 0; rt < 2; rt++)
                a[rt] = *reinterpret_cast<const bf16x8 *>(sF + (rhalf * 64 + rt * 32 + l31) * fstride + ks * 16 + lh * 8);
#pragma unroll
            for (int ct = 0; ct < CTB; ct++) b[ct] = frag(w, (cgrp * CTB + ct) * 32 + l31, lh);
#pragma unroll
            for (int rt = 0; rt < 2; rt++)
#pragma unroll
                for (int ct = 0; ct < CTB; ct++)
                    acc[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[rt], b[ct], acc[rt][ct], 0, 0, 0);
            if (SCORE) {
                const bf16x8 fb = st ? a[1] : a[0]; // B operand: B[k][j = passage]  (same bytes as the A fragment of F)
#pragma unroll
                for (int p = 0; p < 3; p++) {
                    const bf16x8 g = frag(w, DPB + p * 64 + qt * 32 + l31, lh);
                    accs = __builtin_amdgcn_mfma_f32_32x32x16_bf16(g, fb, accs, 0, 0, 0); // C[i = query][j = passage]
                }
            }
        }
        __syncthreads(); // every wave is done with the ring (all DMA waited for: a plain barrier)

        // ---- masked mean pooling over the L token rows of a passage: encode_kernel's arithmetic, per block ----
        if (POOL) {
#pragma unroll
            for (int rt = 0; rt < 2; rt++) {
#pragma unroll
                for (int g4 = 0; g4 < 4; g4++) {
                    const int r0 = rhalf * 64 + rt * 32 + 8 * g4 + 4 * lh;
                    const float m0 = sM[r0], m1 = sM[r0 + 1], m2 = sM[r0 + 2], m3 = sM[r0 + 3];
#pragma unroll
                    for (int ct = 0; ct < CTB; ct++) {
                        float v0 = acc[rt][ct][4 * g4] * m0, v1 = acc[rt][ct][4 * g4 + 1] * m1;
                        float v2 = acc[rt][ct][4 * g4 + 2] * m2, v3 = acc[rt][ct][4 * g4 + 3] * m3;
                        if (L == 1) {
                            v0 /= sC[r0]; v1 /= sC[r0 + 1]; v2 /= sC[r0 + 2]; v3 /= sC[r0 + 3];
                        } else if (L == 2) {
                            v0 = (v0 + v1) / sC[r0]; v2 = (v2 + v3) / sC[r0 + 2]; v1 = 0.f; v3 = 0.f;
                        } else if (L == 4) {
                            v0 = (((v0 + v1) + v2) + v3) / sC[r0]; v1 = v2 = v3 = 0.f;
                        } else { // L == 8: tokens 0-3 in the lane with lh = 0, tokens 4-7 in its lh = 1 partner
                            float s4 = ((v0 + v1) + v2) + v3;
                            float t = s4 + __shfl_xor(s4, 32, 64);
                            v0 = lh == 0 ? t / sC[r0] : 0.f; v1 = v2 = v3 = 0.f;
                        }
                        acc[rt][ct][4 * g4] = v0; acc[rt][ct][4 * g4 + 1] = v1; acc[rt][ct][4 * g4 + 2] = v2; acc[rt][ct][4 * g4 + 3] = v3;
                    }
                }
            }
        }
        // ---- this block's share of the row sums of squares, added by the lane that owns the entry -------------
#pragma unroll
        for (int rt = 0; rt < 2; rt++) {
#pragma unroll
            for (int reg = 0; reg < 16; reg++) {
                float p = 0.f;
#pragma unroll
                for (int ct = 0; ct < CTB; ct++) p = fmaf(acc[rt][ct][reg], acc[rt][ct][reg], p);
                p += __shfl_xor(p, 1, 64);
                p += __shfl_xor(p, 2, 64);
                p += __shfl_xor(p, 4, 64);
                p += __shfl_xor(p, 8, 64);
                p += __shfl_xor(p, 16, 64);
                if (l31 == 0) sN[cgrp * 128 + rhalf * 64 + rt * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lh] += p;
            }
        }
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
                        for (int ct = 0; ct < CTB; ct++) {
                            const uint32_t col = col0 + (cgrp * CTB + ct) * 32 + l31;
                            if (col < ld_out) E[(size_t)(row / L) * ld_out + col] = col < d ? acc[rt][ct][reg] : 0.f;
                        }
                    }
                }
            }
        }
        // ---- SCORE (the last block): score tile, rows (regs) = queries, col (lane & 31) = token row; as encode_kernel ----
        if constexpr (SCORE) {
            __syncthreads(); // the sums of squares of every block and column group are in sN
            const int r = rhalf * 64 + st * 32 + l31;
            const uint64_t row = row_base + r;
            const float ss = ((sN[r] + sN[128 + r]) + (sN[256 + r] + sN[384 + r]));
            float nrm = sqrtf(ss);
            nrm = nrm < 1e-12f ? 1e-12f : nrm;
            if (!POOL) {
                if (row < n) {
#pragma unroll
                    for (int reg = 0; reg < 16; reg++) {
                        const uint32_t q = qt * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
                        if (q < nq) S[(size_t)q * n_rows_s + row] = accs[reg] / nrm;
                    }
                }
            } else {
                const float m = sM[r];
                const bool first = (r % L) == 0;
                const float cnt = first ? sC[r] : 1.f;
#pragma unroll
                for (int reg = 0; reg < 16; reg++) {
                    float v = accs[reg] * m;
                    if (L >= 2) v += __shfl_xor(v, 1, 64);
                    if (L >= 4) v += __shfl_xor(v, 2, 64);
                    if (L >= 8) v += __shfl_xor(v, 4, 64);
                    const uint32_t q = qt * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
                    if (first && row < n && q < nq) S[(size_t)q * n_rows_s + row / L] = (v / cnt) / nrm;
                }
            }
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
            const float ss = ((sN[r] + sN[128 + r]) + (sN[256 + r] + sN[384 + r])); // fixed order: reproducible
            float nrm = sqrtf(ss);
            nrm = nrm < 1e-12f ? 1e-12f : nrm;
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
