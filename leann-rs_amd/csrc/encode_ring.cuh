// encode_ring.cuh — fragment of encode_kernel and encode_blocked_kernel (there inside run_block), included textually
// (profiles/encode_fragments.md): the two accessors of the LDS ring of k-step slabs, and the zeroed accumulators of one block of
// CT * 128 columns.
//   expects: CT, SCORE (the slabs carry the three 64-query pieces of G behind the columns), DP = CT * 128, DPX, NI, PER, Wp, Gp,
//            sW, lane, wave, and from the including site just above the include:
//              dp    the padded columns of the tiled weights Wp[kstep][dp][16] (= DP for the one block)
//              col0  the block's first column (0 for the one block)
//            In encode_blocked_kernel both are the kernel's own: a local copy of dp moved instructions in two of its kernels.
//   defines: stage_w(slot, ks), frag(region, col, lh), acc[2][CT] = 0, accs = 0
//   barriers: none
// k-step staging by LDS-DMA (global_load_lds_dwordx4: 64 lanes x 16 B = 1 KiB per wave instruction, no VGPRs,
// asynchronous until the wave's vmcnt wait).  The LDS image is linear in 16-B slots; slot p holds global piece
// p ^ ((p >> 4) & 1) of the block's column range (swizzle on the SOURCE address), which makes the 32-B-stride fragment reads
// conflict-free.
auto stage_w = [&](int slot, uint32_t ks) {
    const char *wsrc = reinterpret_cast<const char *>(Wp + ((size_t)ks * dp + col0) * 16);
    const char *gsrc = SCORE ? reinterpret_cast<const char *>(Gp + (size_t)ks * 192 * 16) : nullptr;
    char *dst = reinterpret_cast<char *>(sW + slot * DPX * 16);
#pragma unroll
    for (int j = 0; j < PER; j++) {
        uint32_t i = wave + 8 * j;
        if (i >= (uint32_t)NI) i = NI - 1; // padding instruction: re-fetches the last piece (same bytes, same place)
        const uint32_t p = i * 64 + lane, g = p ^ ((p >> 4) & 1);
        const char *src = (!SCORE || g < (uint32_t)(DP * 2)) ? wsrc + (size_t)g * 16 : gsrc + (size_t)(g - DP * 2) * 16;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                         (__attribute__((address_space(3))) void *)(dst + i * 1024), 16, 0, 0);
    }
};
auto frag = [](const uint16_t *region, uint32_t col, int lh) -> bf16x8 { // 8 consecutive k of one column (16 B)
    const uint32_t g = 2 * col + lh, p = g ^ ((g >> 4) & 1);
    return *reinterpret_cast<const bf16x8 *>(reinterpret_cast<const char *>(region) + p * 16);
};
f32x16 acc[2][CT];
f32x16 accs; // SCORE: scores of query tile (cgrp & 1) x passage tile (2*rhalf + (cgrp >> 1))
#pragma unroll
for (int i = 0; i < 16; i++) accs[i] = 0.f;
#pragma unroll
for (int rt = 0; rt < 2; rt++)
#pragma unroll
    for (int ct = 0; ct < CT; ct++)
#pragma unroll
        for (int i = 0; i < 16; i++) acc[rt][ct][i] = 0.f;
