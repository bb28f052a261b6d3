// Not a self-contained header (no include guard): a fragment of beam_search_one (search.cuh), included once in each form of the hop loop.
// Phase C, every wave: distances of the hop's unseen neighbours, R rows in flight per wave (G16: four rows per wave instruction,
// R groups), and their keys; filtered searches also write the copy with the disallowed keys blanked.
// Expects:  lane, wave, NW, R, T, q / qa, qb, g, lv, deg, adj0_p, n_new, filt_level, allow, EARLY_B,
//           snew (the hop's unseen ids), skey, skeyR (where their keys go)
// Writes:   skey[0 .. n_new), skeyR[0 .. n_new) when filt_level.  No barrier.
if constexpr (G16) {
    for (uint32_t jb = 0; jb < n_new; jb += NW * 4 * R) {
        uint32_t ids[R], jj[R], abyte[R];
        bool valid[R];
        float dd[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            jj[r] = jb + (uint32_t)(r * NW + wave) * 4u + (uint32_t)(lane >> 4);
            valid[r] = jj[r] < n_new;
            ids[r] = valid[r] ? snew[jj[r]] : 0u;
            abyte[r] = (filt_level && valid[r] && (lane & 15) == 15) ? allow[ids[r] >> 3] : 0u;
        }
#ifndef LEANN_NO_ADJ_TOUCH
        // adjacency lists of the rows being evaluated (see the row-per-wave form below): lanes 12, 13 of a row touch
        [[maybe_unused]] uint32_t touch = 0;
        if constexpr (EARLY_B)
            if (lv == 0 && valid[0] && (lane & 14) == 12 && (uint32_t)(lane & 1) * 32u < deg)
                touch = adj0_p[(size_t)ids[0] * deg + (uint32_t)(lane & 1) * 32u];
#endif
        group_dist_rows_feat256<R>(qa, qb, reinterpret_cast<const char *>(g.X), g.row_bytes, ids, valid, lane, dd, g.norms);
#ifndef LEANN_NO_ADJ_TOUCH
        if constexpr (EARLY_B) asm volatile("" ::"v"(touch));
#endif
        if ((lane & 15) == 15) {
#pragma unroll
            for (int r = 0; r < R; r++)
                if (valid[r]) {
                    const uint64_t key = make_key(dd[r], ids[r]);
                    skey[jj[r]] = key;
                    if (filt_level) skeyR[jj[r]] = ((abyte[r] >> (ids[r] & 7u)) & 1u) ? key : ~0ull;
                }
        }
    }
} else
for (uint32_t j0 = wave; j0 < n_new; j0 += NW * R) {
    uint32_t ids[R];
    float dd[R];
    int nrows = 0;
#pragma unroll
    for (int r = 0; r < R; r++) {
        uint32_t j = j0 + r * NW;
        if (j < n_new) { ids[r] = snew[j]; nrows = r + 1; }
    }
#ifndef LEANN_NO_ADJ_TOUCH
    // (declared here and not at its use below: in the throughput form it is a dead local, and one that sits between abyte and
    // the row loads changes the order of two register moves in three 4-wave kernels — scripts/device_code_diff.py)
    [[maybe_unused]] uint32_t touch = 0;
#endif
    uint32_t abyte = 0, abit = 0;
    if (filt_level && lane < R && j0 + lane * NW < n_new) { // lane r fetches row r's allow bit alongside the rows
        const uint32_t e = snew[j0 + lane * NW];
        abyte = allow[e >> 3];
        abit = e & 7u;
    }
#ifndef LEANN_NO_ADJ_TOUCH
    // Latency form only: touch the adjacency lists of the rows being evaluated (two 128-B lines each, one lane per
    // line).  The next candidates come from these rows, so when phase E picks one its list is an L2 hit instead of
    // an HBM round trip at the head of the dependent chain; the chip is idle in this mode, the +8 % traffic is free.
    // (An ordinary load issued BEFORE the row loads and consumed behind them: the rows' wait covers it, and the
    // compiler keeps its register reserved until then.)
    if constexpr (EARLY_B)
        if (lv == 0 && (uint32_t)(lane >> 1) < (uint32_t)nrows && (uint32_t)(lane & 1) * 32u < deg)
            touch = adj0_p[(size_t)snew[j0 + (uint32_t)(lane >> 1) * NW] * deg + (uint32_t)(lane & 1) * 32u];
#endif
    if (FEAT) wave_dist_rows_feat<T, R>(q, reinterpret_cast<const char *>(g.X), g.row_bytes, g.feat_h, ids, nrows, lane, dd, g.norms);
    else if constexpr (BF16) wave_dist_rows_bf16<T, R>(q, reinterpret_cast<const uint16_t *>(g.X), g.row_bytes >> 1, ids, nrows, lane, dd);
    else if constexpr (I8) wave_dist_rows_i8<T, R>(q, reinterpret_cast<const int8_t *>(g.X), g.row_bytes, ids, nrows, lane, dd);
    else wave_dist_rows<T, R>(q, g.X, g.ld, ids, nrows, lane, dd);
#ifndef LEANN_NO_ADJ_TOUCH
    if constexpr (EARLY_B) asm volatile("" ::"v"(touch));
#endif
    const unsigned long long amask = FILT ? __ballot((abyte >> abit) & 1u) : 0ull;
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < R; r++)
            if (r < nrows) {
                const uint64_t key = make_key(dd[r], ids[r]);
                skey[j0 + r * NW] = key;
                if (filt_level) skeyR[j0 + r * NW] = ((amask >> r) & 1ull) ? key : ~0ull;
            }
    }
}
