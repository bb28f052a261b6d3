// Not a self-contained header (no include guard): a fragment of beam_search_one (search.cuh), included once in each form of the hop loop.
// Phase E, wave 0: the next candidate, known before the merge.
// The merged beam's first unexpanded entry is the smaller of (a) the first unexpanded entry of the OLD beam other than
// the one just expanded and (b) the smallest new key; its index in the merged beam is the number of keys below it.
// Same entry, same index as a scan of the merged list would give — but available one merge earlier, so wave 0 issues
// the next hop's adjacency load now (in flight across the merge and barrier B3) and the other waves merge meanwhile.
// Expects:  lane, LW, Wc, wsize, sel, ef_l, n_new, skey (this hop's new keys), next_slot, adj_base, upoff_p, deg, lv, stamp (LEANN_STAMPS)
// Defines:  next (the candidate's index in the merged beam, LEANN_EMPTY when the level is finished), ckey (its key)
// Updates:  *next_slot = next; e_pref / e_pref1 = the candidate's adjacency list when there is one.  No barrier.
uint32_t u = LEANN_EMPTY;
for (uint32_t base = 0; base < wsize && u == LEANN_EMPTY; base += 64) {
    const uint32_t i = base + lane;
    const unsigned long long m = __ballot(i < wsize && i != sel && !(Wc[i] & 1ull));
    if (m) u = base + (uint32_t)__ffsll((long long)m) - 1u;
}
const uint64_t c_old = u != LEANN_EMPTY ? Wc[u] : ~0ull;
const uint64_t kj = (uint32_t)lane < n_new ? skey[lane] : ~0ull; // n_new <= 64 LW: LW keys per lane
const uint64_t kj1 = LW == 2 && (uint32_t)lane + 64u < n_new ? skey[lane + 64] : ~0ull;
const uint64_t km = LW == 2 ? min(kj, kj1) : kj;
const uint32_t hi = wave_min_u32((uint32_t)(km >> 32));
const uint32_t lo = wave_min_u32((uint32_t)(km >> 32) == hi ? (uint32_t)km : 0xFFFFFFFFu);
const uint64_t c_new = n_new ? (((uint64_t)hi << 32) | lo) : ~0ull;
uint32_t next = LEANN_EMPTY;
uint64_t ckey = 0;
if (c_old != ~0ull || c_new != ~0ull) {
    uint32_t rank;
    if ((c_old >> 1) < (c_new >> 1)) {
        rank = u + (uint32_t)__popcll(__ballot((kj >> 1) < (c_old >> 1)));
        if constexpr (LW == 2) rank += (uint32_t)__popcll(__ballot((kj1 >> 1) < (c_old >> 1)));
        ckey = c_old;
#ifdef LEANN_STAMPS
        stamp[7] += 1;
#endif
    } else {
        rank = 0;
        for (uint32_t base = 0; base < wsize; base += 64) {
            const uint32_t i = base + lane;
            rank += (uint32_t)__popcll(__ballot(i < wsize && (Wc[i] >> 1) < (c_new >> 1)));
        }
        ckey = c_new;
    }
    if (rank < ef_l) next = rank;
}
if (lane == 0) *next_slot = next;
if (next != LEANN_EMPTY) {
    e_pref = (uint32_t)lane < deg ? adj_list(adj_base, upoff_p, deg, lv, key_id(ckey))[lane] : LEANN_EMPTY;
    if constexpr (LW == 2) e_pref1 = (uint32_t)lane + 64u < deg ? adj_list(adj_base, upoff_p, deg, lv, key_id(ckey))[lane + 64] : LEANN_EMPTY;
}
