// Not a self-contained header (no include guard): a fragment of beam_search_one (search.cuh), included once in each form of the hop loop.
// Phase D, waves 1 .. NW-1 (the caller's `else` of `if (wave == 0)`): merge the beam and the hop's new keys by rank into the other buffer.
// Expects:  tid, NW, Wc, Wn, wsize, n_new, n_pad, sel, ef_l, skey (this hop's new keys, 8 sentinels behind them)
// Writes:   Wn[0 .. min(wsize + n_new, ef_l)); marks entry `sel` expanded (bit 0).  No barrier.
// ---- phase D (waves 1 .. NW-1): merge by rank into the other buffer ---------------------------------
// One work item per old entry (rank = index + #new keys below it) and per new key (rank = #old below it, by
// binary search, + #new below it); the scan over the new keys reads 16 B per LDS instruction, 8 keys per
// unrolled step, so the loads pipeline instead of paying one LDS latency per key.
const ulonglong2 *kp = reinterpret_cast<const ulonglong2 *>(skey);
for (uint32_t it = tid - 64; it < wsize + n_new; it += (NW - 1) * 64) {
    const bool isW = it < wsize;
    uint64_t k = isW ? Wc[it] : skey[it - wsize];
    if (isW && it == sel) k |= 1ull;
    const uint64_t kk = k >> 1;
    uint32_t cnt = 0;
#pragma unroll 4
    for (uint32_t j = 0; j < n_pad; j += 2) {
        const ulonglong2 v = kp[j >> 1];
        cnt += ((v.x >> 1) < kk) + ((v.y >> 1) < kk);
    }
    uint32_t rank = isW ? it + cnt : cnt;
    if (!isW) {
        uint32_t lo = 0, hi = wsize;
        while (lo < hi) {
            uint32_t mid = (lo + hi) >> 1;
            if ((Wc[mid] >> 1) < kk) lo = mid + 1; else hi = mid;
        }
        rank += lo;
    }
    if (rank < ef_l) Wn[rank] = k;
}
