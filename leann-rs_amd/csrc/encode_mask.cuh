// encode_mask.cuh — fragment of encode_kernel and encode_blocked_kernel, included textually (profiles/encode_fragments.md):
// the attention mask of the tile's 128 token rows and the token count of each passage (candle.rs:191-216).
//   expects: POOL, L, mask, n, row_base, tid, sM, sC; whatever the kernel put into LDS before (feature tile, sN) is published too
//   updates: sM[128] (0/1; rows >= n count as padding), sC[first token row of a passage] = max(token count, 1e-9)
//   barriers: one __syncthreads() between the two halves (feature tile + mask visible; no DMA in flight yet: a plain barrier);
//             sC is published by the barriers of the k-loop
if (POOL && tid < 128) {
    const uint64_t row = row_base + tid;
    sM[tid] = (row < n && (!mask || mask[row] != 0)) ? 1.f : 0.f;
}
__syncthreads();
if (POOL && tid < 128 && (tid % L) == 0) {
    float c = 0.f;
    for (uint32_t j = 0; j < L; j++) c += sM[tid + j];
    sC[tid] = c < 1e-9f ? 1e-9f : c; // candle.rs:213 count.clamp(1e-9, inf)
}
