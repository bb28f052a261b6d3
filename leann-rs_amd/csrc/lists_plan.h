// lists_plan.h — the work-unit plan of a search over per-query position lists (scan_lists.hip on f32 rows, scan_lists_i8.hip on int8
// rows).  Plain C++: no device code, no HIP types.
//
// A unit is (list, chunk of LISTS_ROWS listed rows, tile of up to LISTS_QT queries that share the list).  The queries of a slice are
// sorted by list (stable); a list with one query gives lone units, a shared list tiles of LISTS_QT and, if one query is left over, lone
// units for it.  The table holds the lone units first, then the tiled ones: a launch is a flat grid over a range of it.  The slices
// keep a call's candidate buffers — per query, max_chunks x min(k, LISTS_ROWS) keys of 8 bytes, twice — within the scan pool's blocks.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <vector>

constexpr int LISTS_QT = 8;          // queries of one tile of a shared list
constexpr uint32_t LISTS_ROWS = 256; // listed rows of one chunk
struct ListUnit {
    uint64_t off;   // first entry of the chunk in d_lists
    uint32_t cnt;   // entries of the chunk, 1 .. 256
    uint32_t chunk; // chunk number within its list: the slot in cand
    uint32_t q0;    // first query of the tile in ord
    uint32_t nqt;   // queries of the tile, 1 .. QT
};

inline size_t lists_plan_list_of(const uint32_t *q_list, size_t q) { return q_list ? q_list[q] : q; }
inline size_t lists_plan_chunks(const uint64_t *list_off, size_t l) { return (size_t)((list_off[l + 1] - list_off[l] + LISTS_ROWS - 1) / LISTS_ROWS); }

// The slice that starts at query q0: returns its end q1 > q0 and the largest chunk count of its queries.  k keys are kept per query at
// the end, kk = min(k, LISTS_ROWS) per chunk; a lone longer list takes what it needs.
inline size_t lists_plan_slice_end(size_t q0, size_t nq, uint32_t k, const uint64_t *list_off, const uint32_t *q_list, size_t *max_chunks) {
    constexpr size_t CAND_BYTES = (size_t)32 << 20;
    const uint32_t kk = std::min<uint32_t>(k, LISTS_ROWS);
    size_t q1 = q0, mc = 0;
    while (q1 < nq) {
        const size_t c = std::max(mc, lists_plan_chunks(list_off, lists_plan_list_of(q_list, q1)));
        if (q1 > q0 && (q1 - q0 + 1) * std::max<size_t>(c * kk, k) * sizeof(uint64_t) > CAND_BYTES) break;
        mc = c;
        q1++;
    }
    *max_chunks = mc;
    return q1;
}

struct ListsPlan {
    std::vector<uint32_t> ord;   // the slice's queries (0 .. nq - 1, relative to q_base) sorted by list
    std::vector<ListUnit> table; // n_lone lone units, then the tiled ones
    size_t n_lone = 0;
    size_t n_tiled() const { return table.size() - n_lone; }
};
// the units of the slice of nq queries that starts at query q_base
inline ListsPlan lists_plan_units(size_t nq, const uint64_t *list_off, const uint32_t *q_list, size_t q_base) {
    ListsPlan p;
    auto list_of = [&](size_t q) -> size_t { return lists_plan_list_of(q_list, q_base + q); };
    p.ord.resize(nq);
    std::iota(p.ord.begin(), p.ord.end(), 0u);
    std::stable_sort(p.ord.begin(), p.ord.end(), [&](uint32_t a, uint32_t b) { return list_of(a) < list_of(b); });
    std::vector<ListUnit> tiled;
    for (size_t i = 0; i < nq;) {
        const size_t l = list_of(p.ord[i]);
        size_t j = i;
        while (j < nq && list_of(p.ord[j]) == l) j++;
        const uint64_t len = list_off[l + 1] - list_off[l];
        for (size_t t = i; t < j; t += LISTS_QT) {
            const uint32_t nqt = (uint32_t)std::min<size_t>(LISTS_QT, j - t);
            for (uint64_t c = 0; c * LISTS_ROWS < len; c++)
                (nqt == 1 ? p.table : tiled).push_back(ListUnit{list_off[l] + c * LISTS_ROWS, (uint32_t)std::min<uint64_t>(LISTS_ROWS, len - c * LISTS_ROWS),
                                                                (uint32_t)c, (uint32_t)t, nqt});
        }
        i = j;
    }
    p.n_lone = p.table.size();
    p.table.insert(p.table.end(), tiled.begin(), tiled.end());
    return p;
}
