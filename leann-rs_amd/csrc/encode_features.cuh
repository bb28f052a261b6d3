// encode_features.cuh — fragment of encode_kernel and encode_blocked_kernel (recompute.hip, recompute_blocked.cuh), included
// textually at the block's place (profiles/encode_fragments.md): the workgroup's 128 feature rows into sF, zero-padded in rows
// (row >= n) and in k (k >= h), 16 B per thread and step.
//   expects: F, n, h, hp, sF, fstride, row_base, tid
//   updates: sF[128][fstride]
//   barriers: none — the including kernel's next __syncthreads() publishes the tile
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
