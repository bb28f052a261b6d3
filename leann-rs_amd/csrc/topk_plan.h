// topk_plan.h — how an exhaustive top-k (scan.hip: the exact scan and the exact filtered search; recompute.hip: the recompute search)
// cuts its rows into chunks, and what its scratch holds.  Plain C++ on purpose: both searches and the stand-alone host test
// (host/topk_plan_selftest.cpp) compile the same function.  This comment is the one place where the schedules are written down.
//
// Every chunk is scored against all queries of a pass.  A SLAB chunk writes its scores to S [queries x slab_rows]; topk_scores_kernel
// sorts each segment of SEG scores and keeps its k best keys in candA [nq x cand_len], update_best_kernel folds them into the running
// best-k of each query.  An EMITTED chunk writes no scores: the scoring kernel compares each one with the query's running k-th best
// and appends the few that reach it to a per-query list of emit_cap keys (CandEmit, internal.h), which fold_candidates_kernel merges
// into the running best-k.  It needs no slab, no segment and no candidate row.
//
//   emission schedule  chunk 0 is a small slab chunk (emit_first rows, at most slab_cap) that fixes a first k-th best; chunk 1
//                      (emit_second rows) tightens it to ~k * emit_second / emit_first survivors per query; chunk 2 is everything
//                      else, in one launch.  Chunks 1 and 2 are emitted and not capped.  The answer is the running best-k.  A list
//                      that takes more than emit_cap keys (adversarial order, e.g. ascending scores) sets the overflow word, and
//                      the caller repeats the search on the slab schedule.  A schedule of one chunk has nothing to emit: the plan
//                      is then the slab schedule's.
//   slab schedule      geometric slab chunks of 128 Ki rows, then x 4, each at most slab_cap: the first small chunks fix the running
//                      k-th best, after which topk_scores_kernel skips almost every segment unsorted.  The answer is re-derived
//                      from all segment winners.
//
// slab_rows, total_segs and cand_len count slab chunks only: under emission that is chunk 0.
//
// The emission block, one layout for both searches (offsets in bytes; slots = the query slots a scoring kernel reads a threshold for):
//   [0, 4 slots) f32 thr | [4 slots, 8 slots) u32 cnt | u32 overflow at 8 slots | pad to a multiple of 256 | slots x emit_cap u64 list
// so the header holds `slots` floats, `slots` u32 and the flag whatever `slots` is, and the list is aligned to 256 bytes.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <utility>
#include <vector>

#define SEG 2048 // scores per segment of the LDS sorter (bitonic_sort_lds, common.cuh); top_k <= SEG / 2

struct TopkShape {
    size_t n, nq;             // rows (list length when a row list is given), queries of the call
    uint32_t k;
    size_t emit_first, emit_second; // rows of the first two chunks of the emission schedule
    size_t slab_cap;          // most rows of a slab chunk
    size_t q_tile;            // queries per pass over the rows: S holds q_tile x slab_rows scores
    size_t slots;             // threshold / counter slots of the emission block
};
// exact scan: all queries in one pass, so the slab of at most 2^29 scores (2 GiB) caps the chunk
static inline TopkShape topk_shape_scan(size_t n, size_t nq, uint32_t k) {
    const size_t cap = std::max<size_t>(SEG, (((size_t)1 << 29) / std::max<size_t>(nq, 1)) / SEG * SEG);
    return {n, nq, k, (size_t)64 << 10, (size_t)448 << 10, cap, nq, (nq + 63) / 64 * 64}; // score_mfma_kernel: 64-query tiles
}
// recompute search: q_tile queries per pass (FSTAT_MAX_QUERIES with the feature-stationary kernel, the only one that emits; else 64)
static inline TopkShape topk_shape_recompute(size_t n, size_t nq, uint32_t k, size_t q_tile) {
    return {n, nq, k, (size_t)16 << 10, (size_t)496 << 10, (size_t)4 << 20, q_tile, q_tile};
}

struct TopkPlan {
    bool emit = false;                             // the emission schedule is in force
    std::vector<std::pair<size_t, size_t>> chunks; // (row0, rows), contiguous from 0
    size_t slab_rows = SEG, total_segs = 1, cand_len = 0; // the widest slab chunk; segments and candidate keys per query
    uint32_t emit_cap = 0;                         // keys per query list
    size_t slots = 0, cnt_off = 0, overflow_off = 0, list_off = 0, emit_bytes = 0; // the emission block (thr at 0)
    bool slab_chunk(size_t c) const { return !emit || c == 0; }
    bool track_best() const { return chunks.size() > 1; } // one chunk: nothing would read the running best-k
};

// emit: the caller wants the emission schedule (its knobs and its kernel allow it)
static inline TopkPlan topk_plan(const TopkShape &s, bool emit) {
    TopkPlan p;
    for (;; emit = false) {
        p.chunks.clear();
        size_t pos = 0, len = std::min(s.slab_cap, emit ? s.emit_first : (size_t)128 << 10);
        while (pos < s.n) {
            const size_t rows = std::min(len, s.n - pos);
            p.chunks.emplace_back(pos, rows);
            pos += rows;
            if (emit) len = p.chunks.size() == 1 ? s.emit_second : s.n;
            else len = std::min(s.slab_cap, len * 4);
        }
        if (!emit || p.chunks.size() > 1) break;
    }
    p.emit = emit;
    size_t segs = 0;
    for (size_t c = 0; c < p.chunks.size(); c++)
        if (p.slab_chunk(c)) { p.slab_rows = std::max(p.slab_rows, p.chunks[c].second); segs += (p.chunks[c].second + SEG - 1) / SEG; }
    p.total_segs = std::max<size_t>(segs, 1);
    p.cand_len = std::max<size_t>(p.total_segs * s.k, s.k);
    p.emit_cap = std::max<uint32_t>(8192, 32 * s.k); // expected survivors per query ~ k * rows / rows_seen (x19 after 512k of 10M rows)
    p.slots = s.slots;
    p.cnt_off = 4 * s.slots;
    p.overflow_off = 8 * s.slots;
    p.list_off = (p.overflow_off + 4 + 255) / 256 * 256;
    p.emit_bytes = p.list_off + sizeof(uint64_t) * s.slots * p.emit_cap;
    return p;
}
