// search_plan.h — which beam-search kernel a call runs, with how many waves, which visited table and how much LDS: a pure function of
// the index shape, the call and the debug knobs.  Plain C++ on purpose: leann_internal_launch_search (api.hip), the kernel tables of
// api.hip, search_bf16.hip and search_i8.hip and the stand-alone host test (host/search_plan_selftest.cpp, tests/test_cpu_search_plan.py) compile the
// same functions; nothing here needs a GPU.
//
//   family    taken when                 kernel<..>                       width -> T, R                    waves per query (NW)               visited table (hash_bits)
//   F32       stored f32 rows            [wide_]beam_search_kernel        c = ceil(ld / 256) -> T by       16: nq <= 384, 8: nq <= 640,       12 if ld <= 512, ef <= 64, not a
//                                        <T, R, NW, build>,               search_width_T (5 -> 6, 7 -> 8,  else 4; LEANN_DEBUG_NW = v: 16     construction search and no knob,
//                                        [wide_]beam_search_filtered_     9.. -> 12, 13.. -> 16),          (v >= 16), 8 (v >= 8), 4; wide     else pick(ef)
//                                        kernel<T, R, NW>                 R = search_f32_R(T)              lists: 8 -> 16 (no 8-wave form)
//   SCREEN    F32 with NW == 4, T 3 / 6, beam_search_screen_kernel<T, R>  R = LEANN_SCREEN_R3 / _R6        4 (256 work items)                 as F32
//             planes ready, not filtered,
//             not construction, not wide
//   BF16      bf16 rows                  [wide_]bf16_beam_search          T as F32, R = search_bf16_R4(T)  16: nq <= 512 and the width has a  as F32
//                                        [_filtered]_kernel<T, R, NW>     / search_bf16_R16(T)             16-wave form (T < 16), else 4;
//                                                                                                          LEANN_DEBUG_NW is IGNORED
//   I8        int8 rows                  [wide_]i8_beam_search            T as F32, R = search_i8_R4(T)    as BF16 (its threshold: int8       as F32
//                                        [_filtered]_kernel<T, R, NW>     / search_i8_R16(T)               batches were not swept)
//   FEAT      recompute-on graph         [wide_]beam_search_feat          c = ceil(feat_h / 256): <1,      16: nq <= 512, else 4;             knob set: pick(ef); else 12 for
//             (feat_h != 0)              [_filtered]_kernel<T, R, NW>     LEANN_FEAT_R1>, <2, 6>, c = 3    LEANN_DEBUG_NW is IGNORED          ef <= 64, else pick(ef) (at any
//                                                                         and 4: <4, 4>                                                       width, construction refused)
//   FEAT256   FEAT with feat_h == 256    [wide_]beam_search_feat256       <1, 16> (16 waves),              as FEAT                            as FEAT
//             unless LEANN_DEBUG_        [_filtered]_kernel<G, NW>        <LEANN_FEAT_G, 4>
//             NO_FEAT256
//
//   pick(ef): the LEANN_DEBUG_HASH_BITS knob if set, else the smallest b in 13..15 with 2^b >= 24 ef (15 if none).
//   wide: max(M0, M) > 64 (two list ids per lane of wave 0).  LDS: search_lds_bytes(ef, maxdeg, hash_bits, filtered ? k : 0, NW > 4 ? 2 : 1),
//   at most 160 KiB.
// The families disagree on the batch thresholds (384 / 640 against 512) and on LEANN_DEBUG_NW (honoured by F32 alone): each was
// measured on its own workload (scripts/exp/batch_sweep.py, profiles/bf16_rows.md), and this header states the difference, it does
// not settle it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LEANN_SP_HD __host__ __device__
#else
#define LEANN_SP_HD
#endif

// Rows in flight per wave of the screen kernels: a hi-plane row is half a row's bytes (768-d: 4, 1 536-d: 2 as for whole rows).
#ifndef LEANN_SCREEN_R3
#define LEANN_SCREEN_R3 4
#endif
#ifndef LEANN_SCREEN_R6
#define LEANN_SCREEN_R6 2
#endif
// Recompute-on rows of <= 256 features: rows in flight per wave of the 4- and 16-wave kernels (search.cuh: LEANN_FEAT_OCC)
#ifndef LEANN_FEAT_R1
#define LEANN_FEAT_R1 5
#endif
// ... of exactly 256 features: groups of four rows in flight per wave of the 4-wave kernel (search.cuh: LEANN_FEAT256_OCC)
#ifndef LEANN_FEAT_G
#define LEANN_FEAT_G 1
#endif

#define LEANN_SEARCH_LDS_LIMIT ((size_t)160 * 1024)
enum { SEARCH_PLAN_OK = 0, SEARCH_PLAN_INVALID = 1, SEARCH_PLAN_UNSUPPORTED = 5 }; // LEANN_ERR_INVALID / _UNSUPPORTED (leann_backend.h)

// LDS of one query's workgroup (the carve-up: search.cuh, SearchLds).  kf = result-list length of a filtered search (0: unfiltered);
// nbuf = 2 for the latency form of the hop loop (NW > 4: s_key / s_new / s_keyR per hop parity), 1 for the throughput form
LEANN_SP_HD inline size_t search_lds_bytes(uint32_t ef, uint32_t maxdeg, uint32_t hash_bits, uint32_t kf = 0, uint32_t nbuf = 2) {
    size_t efp = (ef + 1) & ~1u;
    size_t b = 2 * efp * 8 + nbuf * ((size_t)maxdeg + 8) * 8 + nbuf * (size_t)maxdeg * 4 + 16 * 4; // s_key carries 8 sentinel slots
    b = (b + 15) & ~(size_t)15;
    if (kf) b += 2 * (size_t)((kf + 1) & ~1u) * 8 + nbuf * ((size_t)maxdeg + 8) * 8;
    return b + ((size_t)1 << hash_bits) * 4;
}

enum SearchFamily { SEARCH_F32 = 0, SEARCH_SCREEN, SEARCH_BF16, SEARCH_FEAT, SEARCH_FEAT256, SEARCH_I8 };

struct SearchShape {
    uint32_t ld, d, feat_h;
    bool bf16;
    uint32_t maxdeg;   // max(M0, M)
    bool screen_ready; // planes in place, the handle's row screen on, and leann_internal_screen_shape
    bool i8 = false;   // int8 rows (rows_i8.hip); never together with bf16 or feat_h
};
struct SearchCall {
    uint32_t nq, k, ef; // ef: already max(ef, k)
    bool filtered, build; // build: a construction search (SearchArgs::q_rows)
};
struct SearchKnobs {
    int hash_bits, nw; // LEANN_DEBUG_HASH_BITS (6..15), LEANN_DEBUG_NW; 0 = unset
    bool no_feat256;   // LEANN_DEBUG_NO_FEAT256
};
struct SearchPlan {
    int family;        // SearchFamily
    int T, R, NW;      // chunks of 256 elements per row, rows (FEAT256: groups of four) in flight per wave, waves per query
    bool wide, filtered, build; // build: the BUILD form of the plain F32 kernel (an allow mask takes the filtered kernel first)
    uint32_t hash_bits;
    size_t lds_bytes;
    int err;           // SEARCH_PLAN_OK, or the refusal and its message
    char msg[120];
};

// ---- the tables: the kernel tables of api.hip and search_bf16.hip instantiate exactly these <T, R> -------------------------------------
// c = chunks of 256 floats in a row -> the compiled width that takes it (the extra chunks read as zeros and add +0 products); 0: none
constexpr int search_width_T(uint32_t c) { return c <= 4 ? (int)c : c <= 6 ? 6 : c <= 8 ? 8 : c <= 12 ? 12 : c <= 16 ? 16 : 0; }
constexpr int search_f32_R(int T) { return T <= 3 ? 4 : T == 4 ? 3 : T <= 8 ? 2 : 1; }
// bf16 rows, 4 / 16 waves per query (how they were chosen: search_bf16.hip); 0: no 16-wave form at this width
constexpr int search_bf16_R4(int T) { return T <= 3 ? 8 : T == 4 ? 6 : T <= 8 ? 4 : 2; }
constexpr int search_bf16_R16(int T) { return T <= 4 ? 4 : T == 6 ? 3 : T == 8 ? 2 : T == 12 ? 1 : 0; }
// int8 rows, 4 / 16 waves per query (how they were chosen: search_i8.hip); 0: no 16-wave form at this width
constexpr int search_i8_R4(int T) { return T == 1 ? 16 : T <= 4 ? 12 : T == 6 ? 8 : T == 8 ? 6 : 4; }
constexpr int search_i8_R16(int T) { return T <= 6 ? 4 : T == 8 ? 3 : T == 12 ? 1 : 0; }
// recompute-on rows: c = chunks of 256 features -> T (0: none), and R by T
constexpr int search_feat_T(uint32_t c) { return c <= 2 ? (int)c : c <= 4 ? 4 : 0; }
constexpr int search_feat_R(int T) { return T == 1 ? LEANN_FEAT_R1 : T == 2 ? 6 : 4; }

// LDS visited table: 4 workgroups per CU are register-limited anyway, so 32 KiB (8192 slots) per query is free; larger beams take
// 64 / 128 KiB.  A query that outgrows it moves to the HBM pool.
static inline uint32_t search_pick_hash_bits(uint32_t ef, int knob) {
    if (knob) return (uint32_t)knob; // test hook: force tiny tables to exercise the HBM pool
    // measured on 10M x 768: ~20-25 distance evaluations per unit of ef on average, p99.9 ~ 50 x ef.
    // 4 workgroups per CU need <= 32 KiB tables; a 64 KiB table halves occupancy and throughput, so
    // beams up to 256 keep the 8 192-slot table and let the ~1 % heaviest queries migrate to HBM.
    uint32_t want = ef * 24u, b = 13;
    while ((1u << b) < want && b < 15) b++;
    return b;
}

static inline SearchPlan search_plan(const SearchShape &s, const SearchCall &c, const SearchKnobs &kn) {
    SearchPlan p = {};
    p.wide = s.maxdeg > 64;
    p.filtered = c.filtered;
    if (s.feat_h) {
        if (c.build) {
            snprintf(p.msg, sizeof p.msg, "recompute-on index: construction searches are not supported");
            p.err = SEARCH_PLAN_UNSUPPORTED;
            return p;
        }
        // 520-B rows make this mode latency- rather than bandwidth-bound: favour occupancy (16 KiB visited table ->
        // 6-8 workgroups per CU) for narrow beams; heavier queries migrate to the HBM pool
        p.hash_bits = !kn.hash_bits && c.ef <= 64 ? 12u : search_pick_hash_bits(c.ef, kn.hash_bits);
        p.T = search_feat_T((s.feat_h + 255) / 256);
        if (!p.T) {
            snprintf(p.msg, sizeof p.msg, "recompute-on index: feature width %u > 1024 not supported", s.feat_h);
            p.err = SEARCH_PLAN_INVALID;
            return p;
        }
        p.NW = c.nq <= 512 ? 16 : 4; // small batches: 16 waves per query, else 4
        if (s.feat_h == 256 && !kn.no_feat256) { // four rows per wave instruction
            p.family = SEARCH_FEAT256;
            p.R = p.NW == 16 ? 1 : LEANN_FEAT_G;
        } else {
            p.family = SEARCH_FEAT;
            p.R = search_feat_R(p.T);
        }
    } else {
        if ((s.bf16 || s.i8) && c.build) {
            snprintf(p.msg, sizeof p.msg, "%s rows: construction searches are not supported", s.i8 ? "int8" : "bf16");
            p.err = SEARCH_PLAN_UNSUPPORTED;
            return p;
        }
        // Rows of up to 512 floats leave registers for 5-7 workgroups per CU where the 32 KiB visited table allows 4, and rows this short
        // do not hide a hop's dependent phases behind their own transfer: narrow beams take the 16 KiB table (the heaviest queries
        // move to the HBM pool).  10M rows, ef = 64: 128-d 2.41 -> 3.10 M queries/s, 256-d 2.16 -> 2.72 M, 384-d 1.66 -> 1.85 M, 512-d
        // unchanged; 768-d and wider are bound by HBM either way and keep the larger table (scripts/exp/dims_sweep.py).
        p.hash_bits = (s.ld <= 512 && c.ef <= 64 && !c.build && !kn.hash_bits) ? 12u : search_pick_hash_bits(c.ef, kn.hash_bits);
        p.T = search_width_T((s.ld + 255) / 256); // 12: 3 072-d, text-embedding-3-large (embedding/models.rs:113)
        if (!p.T) {
            snprintf(p.msg, sizeof p.msg, "search: dims %u > 4096 not supported", s.d);
            p.err = SEARCH_PLAN_INVALID;
            return p;
        }
        if (s.bf16) {
            p.family = SEARCH_BF16;
            p.NW = search_bf16_R16(p.T) && c.nq <= 512 ? 16 : 4;
            p.R = p.NW == 16 ? search_bf16_R16(p.T) : search_bf16_R4(p.T);
        } else if (s.i8) { // the BF16 batch threshold: int8 batches were not swept on their own
            p.family = SEARCH_I8;
            p.NW = search_i8_R16(p.T) && c.nq <= 512 ? 16 : 4;
            p.R = p.NW == 16 ? search_i8_R16(p.T) : search_i8_R4(p.T);
        } else {
            // Waves per query: 4 for throughput batches (4 workgroups per CU hide each other's dependent hops); 16 for small batches,
            // where the chip is mostly idle and the per-hop row fetch is the critical path — all ~40 new rows of a hop are then in
            // flight at once (results are identical: same order, same sums).  10M x 768, ef = 56: 16 waves win up to 256 queries, 8 at
            // 512, 4 from 768 on (scripts/exp/batch_sweep.py)
            int nw = c.nq <= 384 ? 16 : c.nq <= 640 ? 8 : 4;
            if (kn.nw) nw = kn.nw;
            // wide lists exist in the 4- and 16-wave forms only (the 8-wave form's batches run 16 waves): every wide form adds the
            // compile time of a narrow one
            if (nw >= 8 && p.wide) nw = 16;
            p.NW = nw >= 16 ? 16 : nw >= 8 ? 8 : 4;
            p.build = c.build && !c.filtered;
            p.family = SEARCH_F32;
            p.R = search_f32_R(p.T);
            // the handle's split planes are in place: the plain throughput form takes the row-screen kernel.  The latency forms, the
            // filtered and the construction searches read whole rows
            if (p.NW == 4 && (p.T == 3 || p.T == 6) && s.screen_ready && !c.filtered && !c.build && !p.wide) {
                p.family = SEARCH_SCREEN;
                p.R = p.T == 3 ? LEANN_SCREEN_R3 : LEANN_SCREEN_R6;
            }
        }
    }
    p.lds_bytes = search_lds_bytes(c.ef, s.maxdeg, p.hash_bits, c.filtered ? c.k : 0u, p.NW > 4 ? 2u : 1u);
    if (p.lds_bytes > LEANN_SEARCH_LDS_LIMIT) {
        snprintf(p.msg, sizeof p.msg, "search: complexity %u needs %zu B of LDS per query (> 160 KiB)", c.ef, p.lds_bytes);
        p.err = SEARCH_PLAN_INVALID;
    }
    return p;
}

// the kernel's name as a profiler prints it, e.g. "beam_search_kernel<3, 4, 16, false>"
static inline int search_plan_name(const SearchPlan &p, char *buf, size_t cap) {
    const char *w = p.wide ? "wide_" : "", *f = p.filtered ? "_filtered" : "";
    switch (p.family) {
        case SEARCH_F32:
            if (p.filtered) return snprintf(buf, cap, "%sbeam_search_filtered_kernel<%d, %d, %d>", w, p.T, p.R, p.NW);
            return snprintf(buf, cap, "%sbeam_search_kernel<%d, %d, %d, %s>", w, p.T, p.R, p.NW, p.build ? "true" : "false");
        case SEARCH_SCREEN: return snprintf(buf, cap, "beam_search_screen_kernel<%d, %d>", p.T, p.R);
        case SEARCH_BF16: return snprintf(buf, cap, "%sbf16_beam_search%s_kernel<%d, %d, %d>", w, f, p.T, p.R, p.NW);
        case SEARCH_I8: return snprintf(buf, cap, "%si8_beam_search%s_kernel<%d, %d, %d>", w, f, p.T, p.R, p.NW);
        case SEARCH_FEAT: return snprintf(buf, cap, "%sbeam_search_feat%s_kernel<%d, %d, %d>", w, f, p.T, p.R, p.NW);
        case SEARCH_FEAT256: return snprintf(buf, cap, "%sbeam_search_feat256%s_kernel<%d, %d>", w, f, p.R, p.NW);
        default: return snprintf(buf, cap, "(no kernel family %d)", p.family);
    }
}
