// encode_kloop.cuh — fragment of encode_kernel and encode_blocked_kernel (there inside run_block), included textually
// (profiles/encode_fragments.md): the GEMM of one block of CT * 128 columns over all k-steps, through the 3-slot LDS-DMA ring.
//   expects: everything encode_ring.cuh expects and defines, RING, nks, sF, fstride, l31, lh, rhalf, cgrp, st, qt; the ring free
//            and no vector memory operation of this wave outstanding other than what the loop issues (the counted waits count
//            DMA instructions only)
//   updates: acc[2][CT] += F W over the block's columns; SCORE: accs += G F^T (3 MFMAs per k-step, hi / lo / lo2 pieces, for one
//            32-query x 32-passage score tile, the feature fragment reused as the B operand)
//   barriers: one raw s_barrier per k-step behind a counted vmcnt wait; all DMA is waited for at the last k-step.  The barrier
//             that lets the next phase reuse the ring is the including site's.
stage_w(0, 0);
if (nks > 1) stage_w(1, 1);
for (uint32_t ks = 0; ks < nks; ks++) {
    // (a) my pieces of slab ks have landed (slab ks+1 may stay in flight), (b) everybody's have, and everybody
    // is done reading slab ks-1, so (c) its slot can take slab ks+2.  One raw barrier per k-step; __syncthreads()
    // would drain the DMA queue (vmcnt(0)) and serialise the stream.
    if (ks + 1 < nks) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (ks + 2 < nks) stage_w((ks + 2) % RING, ks + 2);
    const uint16_t *w = sW + (ks % RING) * DPX * 16;
    bf16x8 a[2], b[CT];
#pragma unroll
    for (int rt = 0; rt < 2; rt++)
        a[rt] = *reinterpret_cast<const bf16x8 *>(sF + (rhalf * 64 + rt * 32 + l31) * fstride + ks * 16 + lh * 8);
#pragma unroll
    for (int ct = 0; ct < CT; ct++) b[ct] = frag(w, (cgrp * CT + ct) * 32 + l31, lh);
#pragma unroll
    for (int rt = 0; rt < 2; rt++)
#pragma unroll
        for (int ct = 0; ct < CT; ct++)
            acc[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[rt], b[ct], acc[rt][ct], 0, 0, 0);
    if (SCORE) {
        const bf16x8 fb = st ? a[1] : a[0]; // B operand: B[k][j = passage]  (same bytes as the A fragment of F)
#pragma unroll
        for (int p = 0; p < 3; p++) {
            const bf16x8 g = frag(w, DP + p * 64 + qt * 32 + l31, lh);
            accs = __builtin_amdgcn_mfma_f32_32x32x16_bf16(g, fb, accs, 0, 0, 0); // C[i = query][j = passage]
        }
    }
}
