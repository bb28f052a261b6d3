// encode_pool.cuh — fragment of encode_kernel and encode_blocked_kernel (there inside run_block, once per column block), included
// textually (profiles/encode_fragments.md): masked mean pooling of the accumulators over the L token rows of a passage
// (candle.rs:191-216), then the row sums of squares of the pooled values over the block's columns (candle.rs:218-225).
//   expects: POOL, L, CT, acc[2][CT], sM, sC, sN, l31, lh, rhalf, cgrp, all waves past the k-loop's closing barrier, and from the
//            including site just above the include:
//              SN_ADD  constexpr bool: false: sN = this block's sum (the one block); true: sN += it (block after block, by the one
//                      lane that owns the entry: no atomics, the same input gives the same bits)
//   updates: acc (POOL: the pooled mean in the register of the passage's first token, 0 in the others),
//            sN[column group][row]: fmaf over the block's tiles, 5-step butterfly over the 32 lanes of a tile
//   barriers: none — the including site's next __syncthreads() publishes sN
// C/D layout: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5): the four registers of a
// group are four consecutive token rows, so L <= 4 pools in registers and L = 8 adds the lane + 32 partner.
if (POOL) {
#pragma unroll
    for (int rt = 0; rt < 2; rt++) {
#pragma unroll
        for (int g4 = 0; g4 < 4; g4++) {
            const int r0 = rhalf * 64 + rt * 32 + 8 * g4 + 4 * lh;
            const float m0 = sM[r0], m1 = sM[r0 + 1], m2 = sM[r0 + 2], m3 = sM[r0 + 3];
#pragma unroll
            for (int ct = 0; ct < CT; ct++) {
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
#pragma unroll
for (int rt = 0; rt < 2; rt++) {
#pragma unroll
    for (int reg = 0; reg < 16; reg++) {
        float p = 0.f;
#pragma unroll
        for (int ct = 0; ct < CT; ct++) p = fmaf(acc[rt][ct][reg], acc[rt][ct][reg], p);
        // sum over the 32 lanes that share lane >> 5 (the 32 columns of a tile)
        p += __shfl_xor(p, 1, 64);
        p += __shfl_xor(p, 2, 64);
        p += __shfl_xor(p, 4, 64);
        p += __shfl_xor(p, 8, 64);
        p += __shfl_xor(p, 16, 64);
        if (l31 == 0) {
            float &sn = sN[cgrp * 128 + rhalf * 64 + rt * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lh];
            sn = SN_ADD ? sn + p : p;
        }
    }
}
