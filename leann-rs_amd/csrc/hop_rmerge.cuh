// Not a self-contained header (no include guard): a fragment of beam_search_one (search.cuh), included once in each form of the hop loop.
// Filtered searches, every wave (the caller's `if (filt_level)`): the R list takes in the hop's allowed new keys.
// Expects:  tid, lane, NW, R0, kf, kfp, rsize, rcur, n_new, n_pad, skeyR (the new keys, disallowed ones blanked, 8 sentinels behind them)
// Updates:  the other R buffer, rsize, rcur.  No barrier.
// R <- kf best of R ∪ {allowed new keys}: the same merge by rank, on the blanked copy of the new keys.
// Skipped (uniformly) when no allowed new key beats the current kf-th.
uint64_t *Rc = R0 + rcur * kfp, *Rn = R0 + (rcur ^ 1) * kfp;
const uint64_t thr = rsize == kf ? Rc[kf - 1] : ~0ull;
uint32_t n_in = 0;
for (uint32_t j = 0; j < n_new; j += 64) n_in += __popcll(__ballot(j + lane < n_new && skeyR[j + lane] < thr));
if (n_in) {
    const ulonglong2 *kr = reinterpret_cast<const ulonglong2 *>(skeyR);
    for (uint32_t it = tid; it < rsize + n_new; it += NW * 64) {
        const bool isR = it < rsize;
        const uint64_t k = isR ? Rc[it] : skeyR[it - rsize];
        if (k >= thr && !isR) continue; // disallowed, or cannot enter a full list
        uint32_t cnt = 0;
#pragma unroll 4
        for (uint32_t j = 0; j < n_pad; j += 2) {
            const ulonglong2 v = kr[j >> 1];
            cnt += (v.x < k) + (v.y < k);
        }
        uint32_t rank = isR ? it + cnt : cnt;
        if (!isR) {
            uint32_t lo = 0, hi = rsize;
            while (lo < hi) {
                uint32_t mid = (lo + hi) >> 1;
                if (Rc[mid] < k) lo = mid + 1; else hi = mid;
            }
            rank += lo;
        }
        if (rank < kf) Rn[rank] = k;
    }
    rsize = min(rsize + n_in, kf);
    rcur ^= 1;
}
