// meta_batch_plan.h — how a batch of metadata filters (one per output bitmap) becomes the launches of meta_eval_batch_kernel (meta.hip).
// Plain C++ on purpose, no HIP, like meta_plan.h: meta.hip and the stand-alone host test (host/meta_batch_selftest.cpp) compile the
// same planner, and the selftest runs a planned launch with the scalar interpreter at the end of this file.
//
// Every filter is compiled by meta_compile as it is for a single evaluation.  Two filters are the same PROGRAM when their compiled
// MetaProgram and their words are byte-equal (meta_compile zeroes the struct first, so memcmp is sound): a program shared by several
// outputs is evaluated once per 64 rows and its answer written to each of them.  A LAUNCH holds
//   - up to MB_MAX_PROGRAMS distinct programs,
//   - a union column table of up to MB_MAX_COLS store columns — each column the launch's programs name, once; a program's col_id[s]
//     is rewritten from the store's column to its slot in that table, so the kernel reads a column once per step for all programs,
//   - one words block of up to MP_MAX_WORDS words: the programs' number sets and bitsets one behind the other.  set_off is rebased for
//     MP_NUM_IN / MP_NUM_NOT_IN, str_a for MP_STR_BITSET / MP_STR_NOT_BITSET only (for the range ops str_a is a dictionary bound, not
//     an offset).  Every program's words have an even length, so sets stay 8-byte aligned,
//   - the (output, program) pairs it writes.
// Programs are packed greedily in the order of their first appearance; a new launch starts when the next program would exceed one
// of the three caps.  One filter always fits an empty launch by meta_plan.h's own limits (MP_MAX_COLS <= MB_MAX_COLS fields, at most
// MP_MAX_WORDS words), so a batch is never refused for its size — only for what meta_compile refuses in one of its filters, and then
// with meta_compile's message behind "filter <index>: ".
#pragma once
#include "meta_plan.h"
#include <map>

#define MB_MAX_PROGRAMS 64
#define MB_MAX_COLS 16

struct MetaBatchPair {
    uint32_t out, prog; // bitmap `out` of the batch = program `prog` of this launch
};
struct MetaBatchLaunch {
    std::vector<MetaProgram> programs; // col_id: slots of `cols`; set_off / str_a: offsets into `words`
    std::vector<uint16_t> cols;        // the union column table: the store's column behind each slot
    uint8_t col_need[MB_MAX_COLS];     // per slot, the OR of the programs' col_need: bit 0 numbers are tested, bit 1 codes
    std::vector<uint32_t> words;
    std::vector<MetaBatchPair> pairs;
};
struct MetaBatchPlan {
    std::vector<MetaBatchLaunch> launches;
    size_t n_distinct = 0; // programs over all launches
};

// nodes + node_off [n_out + 1]: filter i is nodes[node_off[i] .. node_off[i + 1]), prefix order (node_off[0] == 0, monotone: the
// caller's to check).  index_base is added to the filter index of an error message (a caller that plans a long batch in chunks).
// LEANN_OK, or LEANN_ERR_INVALID with *err = "filter <i>: <meta_compile's message>"; *plan is then unspecified.
inline int meta_batch_plan(const leann_meta_node *nodes, const size_t *node_off, size_t n_out, const std::vector<MetaColumnRef> &columns,
                           MetaBatchPlan *plan, std::string *err, size_t index_base = 0) {
    plan->launches.clear();
    plan->n_distinct = 0;
    struct Where { uint32_t launch, prog; };
    std::map<std::string, Where> seen; // program bytes + words bytes -> where it was packed
    MetaProgram P;
    std::vector<uint32_t> words;
    std::string key;
    for (size_t o = 0; o < n_out; o++) {
        std::string msg;
        if (meta_compile(nodes + node_off[o], node_off[o + 1] - node_off[o], columns, &P, &words, &msg) != LEANN_OK) {
            *err = "filter " + std::to_string(index_base + o) + ": " + msg;
            return LEANN_ERR_INVALID;
        }
        key.assign(reinterpret_cast<const char *>(&P), sizeof P);
        key.append(reinterpret_cast<const char *>(words.data()), words.size() * 4);
        auto it = seen.find(key);
        if (it != seen.end()) {
            plan->launches[it->second.launch].pairs.push_back(MetaBatchPair{(uint32_t)o, it->second.prog});
            continue;
        }
        // does it fit the launch being filled?  columns it would add to the union table:
        auto new_cols = [&](const MetaBatchLaunch &L) {
            size_t add = 0;
            for (uint32_t s = 0; s < P.n_cols; s++) add += std::find(L.cols.begin(), L.cols.end(), P.col_id[s]) == L.cols.end();
            return add;
        };
        if (plan->launches.empty() || plan->launches.back().programs.size() == MB_MAX_PROGRAMS ||
            plan->launches.back().cols.size() + new_cols(plan->launches.back()) > MB_MAX_COLS ||
            plan->launches.back().words.size() + words.size() > MP_MAX_WORDS) {
            plan->launches.emplace_back();
            memset(plan->launches.back().col_need, 0, sizeof plan->launches.back().col_need);
        }
        MetaBatchLaunch &L = plan->launches.back();
        const uint32_t base = (uint32_t)L.words.size(); // even: every program's words have an even length
        for (uint32_t s = 0; s < P.n_cols; s++) {
            size_t u = std::find(L.cols.begin(), L.cols.end(), P.col_id[s]) - L.cols.begin();
            if (u == L.cols.size()) L.cols.push_back(P.col_id[s]);
            P.col_id[s] = (uint16_t)u;
            L.col_need[u] |= P.col_need[s];
        }
        for (uint32_t i = 0; i < P.n_cond; i++) {
            MetaCond &k = P.cond[i];
            if (k.num_op == MP_NUM_IN || k.num_op == MP_NUM_NOT_IN) k.set_off += base;
            if (k.str_op == MP_STR_BITSET || k.str_op == MP_STR_NOT_BITSET) k.str_a += base;
        }
        L.words.insert(L.words.end(), words.begin(), words.end());
        seen.emplace(key, Where{(uint32_t)(plan->launches.size() - 1), (uint32_t)L.programs.size()});
        L.pairs.push_back(MetaBatchPair{(uint32_t)o, (uint32_t)L.programs.size()});
        L.programs.push_back(P);
        plan->n_distinct++;
    }
    return LEANN_OK;
}

// One row and one program of a planned launch, on the host: tag / num / code [slot] are the row's entries in the launch's UNION
// columns (L.cols).  As the kernel does, a number / code is handed to the program only where the tag says so and the launch tests it.
inline bool meta_batch_eval_row(const MetaBatchLaunch &L, uint32_t prog, const uint8_t *tag, const double *num, const uint32_t *code) {
    const MetaProgram &P = L.programs[prog];
    uint8_t t[MP_MAX_COLS];
    double x[MP_MAX_COLS];
    uint32_t c[MP_MAX_COLS];
    for (uint32_t s = 0; s < P.n_cols; s++) {
        const uint32_t u = P.col_id[s];
        t[s] = tag[u];
        x[s] = t[s] == LEANN_META_NUMBER && (L.col_need[u] & 1) ? num[u] : 0.0;
        c[s] = t[s] == LEANN_META_STRING && (L.col_need[u] & 2) ? code[u] : 0u;
    }
    return meta_eval_row(P, L.words.data(), t, x, c);
}
