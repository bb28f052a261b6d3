// encode_score.cuh — fragment of encode_kernel (FUSED) and of encode_blocked_kernel's last block (SCORE), included textually
// (profiles/encode_fragments.md): the score epilogue, S[q][passage] = <mean, q> / ||mean||.
//   expects: accs, POOL, L, n, nq, S, n_rows_s, row_base, sN, sM, sC, l31, lh, rhalf, st, qt; sN complete and published (the
//            including site's __syncthreads() in front of the include)
//   updates: S
//   barriers: none
// score tile: rows (regs) = queries, col (lane & 31) = token row.  Mask, pool the L adjacent lanes of a
// passage, then <mean, q> / ||mean||; 128-B coalesced stores into S[q][passage] when L = 1.
const int r = rhalf * 64 + st * 32 + l31;
const uint64_t row = row_base + r;
#include "encode_norm.cuh"
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
