// Not a self-contained header (no include guard): a fragment of beam_search_one (search.cuh), included once in each form of the hop loop.
// The visited table is full: move the visited set one level up (LDS -> pool 1 -> pool 2).  The caller then redoes phase B of this hop.
// Entered by the WHOLE workgroup (the flag misc[3] is workgroup-uniform), inside the hop loop: `break` leaves that loop.
// Expects:  tid, NW, za, s.misc, table, hsize, hbm, gtab, gbits, gslot, gen, vis_limit, aborted
// Updates:  hbm, gtab, gbits, gslot, gen (LDS -> pool 1 only: pool 1 -> 2 keeps the generation), vis_limit; clears misc[3];
//           sets `aborted` and breaks when there is no level left (defensive: see the pool comment above beam_search_one)
// Barriers: three __syncthreads() (flag read | slot published | new table filled), and a fourth on the pool 1 -> 2 branch before the
//           old table's lock is released.  Holds an in-kernel lock from the CAS on; the epilogue releases it.
const uint32_t next = hbm + 1;
if (next > 2 || (next == 2 && !za->gpool2)) { aborted = true; break; } // defensive: see the pool comment above
__syncthreads(); // every thread has read the flag before it is cleared
if (tid == 0) {
    uint32_t *locks = next == 1 ? za->gpool_lock : za->gpool2_lock;
    const uint32_t ntab = next == 1 ? za->gpool_tables : za->gpool2_tables;
    uint32_t t = atomicAdd(&za->gpool_ctr[next == 1 ? 0 : 2], 1u), slot;
    for (uint32_t i = 0;; i++) { // holders never wait for anything, so a table always comes free
        slot = (t + i) % ntab;
        if (atomicCAS(&locks[slot], 0u, 1u) == 0u) break;
        if ((i % ntab) == ntab - 1) __builtin_amdgcn_s_sleep(32);
    }
    s.misc[4] = slot;
    if (!hbm) s.misc[5] = atomicAdd(&za->gpool_ctr[1], 1u) + 1u; // pool 1 -> 2 keeps the generation
    s.misc[3] = 0;
}
__syncthreads();
const uint32_t nslot = uni(s.misc[4]);
const uint32_t nbits = next == 1 ? za->gpool_bits : za->gpool2_bits;
unsigned long long *ntab_p = (next == 1 ? za->gpool : za->gpool2) + ((size_t)nslot << nbits);
if (!hbm) {
    gen = uni(s.misc[5]);
    for (uint32_t i = tid; i < hsize; i += NW * 64) {
        uint32_t e = table[i];
        if (e != LEANN_EMPTY) vis_insert_hbm(ntab_p, nbits, gen, e);
    }
} else {
    for (uint32_t i = tid; i < (1u << gbits); i += NW * 64) {
        const unsigned long long cur_e = __hip_atomic_load(&gtab[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((uint32_t)(cur_e >> 32) == gen) vis_insert_hbm(ntab_p, nbits, gen, (uint32_t)cur_e);
    }
    __syncthreads(); // every probe of the old table has returned
    if (tid == 0) atomicExch(&za->gpool_lock[gslot], 0u);
}
gtab = ntab_p;
gbits = nbits;
gslot = nslot;
hbm = next;
vis_limit = (1u << gbits) - (1u << (gbits - 2));
__syncthreads();
