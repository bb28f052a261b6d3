// Not a self-contained header (no include guard): a fragment of beam_search_one (search.cuh), included once in each form of the hop loop.
// Phase B, wave 0: the adjacency list of the node being expanded (prefetched into e_pref / e_pref1) goes through the visited table;
// the unseen ids are compacted into the hop's id list.  With the table too full for a whole list nothing is inserted and the
// overflow flag goes up instead: the workgroup migrates the table (hop_migrate.cuh) and this phase runs again for the same node.
// Expects:  lane, LW, EARLY_B, s, kstride, maxdeg, s_keyR, za, a, qi, lv, deg, filt_level, e_pref, e_pref1,
//           hbm, gtab, gbits, gen, table, hbits, vis_limit,
//           p (parity of the hop's buffers: 0 in the throughput form), ckey (key of the node), hidx (index of the hop)
// Updates:  n_vis, n_evals, hops0 / hopsU; s_new and the 8 sentinel keys of parity p; the hop's count in misc[0] (throughput form)
//           or misc[8 + p] (latency form); misc[3] = 1 on overflow.  No barrier.
uint64_t *skey = s.s_key + p * kstride;
uint32_t *snew = s.s_new + p * maxdeg;
const uint32_t node = key_id(ckey);
if (za->out_expanded && lv == (int)a.target_level && lane == 0 && hidx < za->exp_cap)
    za->out_expanded[(size_t)qi * za->exp_cap + hidx] = ((ckey >> 32) << 32) | node;
uint32_t n_new = 0;
const bool ovf = (n_vis + deg > vis_limit);
if (!ovf) {
    const uint32_t e = e_pref; // this node's list (a hop redone after a table migration reads the same register again)
    bool isnew = false;
    if (e != LEANN_EMPTY) isnew = hbm ? vis_insert_hbm(gtab, gbits, gen, e) : vis_insert_lds(table, hbits, e);
    const unsigned long long m = __ballot(isnew);
    const uint32_t pos = __popcll(m & ((1ull << lane) - 1ull));
    if (isnew) snew[pos] = e;
    n_new = __popcll(m);
    if constexpr (LW == 2) { // ids 64..127: a second ballot, compacted behind the first half's unseen ids
        const uint32_t e1 = e_pref1;
        bool isnew1 = false;
        if (e1 != LEANN_EMPTY) isnew1 = hbm ? vis_insert_hbm(gtab, gbits, gen, e1) : vis_insert_lds(table, hbits, e1);
        const unsigned long long m1 = __ballot(isnew1);
        if (isnew1) snew[n_new + __popcll(m1 & ((1ull << lane) - 1ull))] = e1;
        n_new += __popcll(m1);
    }
}
n_vis += n_new;
n_evals += n_new;
if (!ovf) { if (lv == 0) hops0++; else hopsU++; }
if (lane < 8) skey[n_new + lane] = ~0ull; // sentinels: the merge scans keys 8 at a time
if (filt_level && lane < 8) (s_keyR + p * kstride)[n_new + lane] = ~0ull;
if (lane == 0) {
    s.misc[EARLY_B ? 8 + p : 0] = n_new;
    if (ovf) s.misc[3] = 1;
}
