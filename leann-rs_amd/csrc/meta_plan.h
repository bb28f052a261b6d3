// meta_plan.h — how a metadata filter (src/index/filter.rs:328-418 of the reference: FilterCondition::matches, values_equal,
// compare_values) becomes the small program meta_eval_kernel (meta.hip) runs over a columnar store.  Plain C++ on purpose, no HIP:
// meta.hip and the stand-alone host test (host/meta_plan_selftest.cpp) compile the same compiler and the same two row tests; the
// selftest runs the program with the scalar interpreter at the end of this file.  This comment is the one place where the reduction
// is written down.
//
// A column holds per row a tag (LEANN_META_MISSING .. LEANN_META_OTHER), a number (NUMBER rows) and a code (STRING rows): the index of
// the row's string in the column's dictionary, the distinct strings sorted bytewise ascending (a proper prefix first), so code order is
// Rust's str::cmp order.  Every condition of the reference reduces to one form per row:
//
//     match = tag_mask bit `tag`  OR  (tag == NUMBER and num_test(num))  OR  (tag == STRING and str_test(code))
//
//   num_test: never, < c, <= c, > c, >= c, |x - c| < DBL_EPSILON (values_equal), its negation, member / non-member of a set of
//             numbers under that same equality.
//   str_test: never, lo <= code < hi, its negation, bit `code` of a bitset over the dictionary, its negation.
//   ("always" is the tag's bit in tag_mask with the test `never`.)
//
// lb(s) / ub(s): the number of dictionary entries < s / <= s.  P = every present tag (all but MISSING), A = P + MISSING,
// N / S = the NUMBER / STRING bit.  `other` = a value that is neither (null, bool, list).
//
//   op          value     tag_mask              num_test      str_test
//   Exists      any       P                     -             -
//   Eq          null      NULL bit              -             -
//   Eq          bool      FALSE / TRUE bit      -             -
//   Eq          number c  0                     == c          -
//   Eq          string s  0                     -             [lb(s), ub(s))
//   Eq          list      0                     -             -               (values_equal is typed: a list equals nothing)
//   Ne          v         A minus Eq's bits, minus N / S where Eq has a test; the test negated   (Ne is true on MISSING)
//   Gt / Lt     number c  0                     > c / < c     -
//   Gt / Lt     string s  0                     -             [ub(s), D) / [0, lb(s))
//   Gt / Lt     other     0                     -             -               (compare_values gives 0)
//   Gte / Lte   number c  P - N                 >= c / <= c   -               (0 for every present row of another type: true)
//   Gte / Lte   string s  P - S                 -             [lb(s), D) / [0, ub(s))
//   Gte / Lte   other     P                     -             -
//   In          list      bits of its nulls / bools; number set of its numbers; one string: its Eq range, more: a bitset
//   In          no list   0                     -             -
//   NotIn       list      A minus In's bits, minus N / S where In has a test; the test negated
//   NotIn       no list   A
//   StartsWith  p         0                     -             [lb(p), lb(succ(p)))   succ(p): trailing 0xFF bytes dropped, the last
//                                                             remaining byte + 1; an empty or all-0xFF p runs to D
//   Contains /  p         0                     -             bitset from ONE host pass over the dictionary (not over the rows);
//   EndsWith                                                  an empty p: [0, D)
//   (a pattern op whose value is no string uses the empty pattern: as_str().unwrap_or(""))
//
// The tree is compiled to a stack program over wave-wide condition masks.  Slot 0 of the stack is the answer and starts as an OR
// frame; a node acts on the top frame by its PARENT's kind:  COND_AND i / COND_OR i: top &= / |= mask of condition i;  PUSH_AND /
// PUSH_OR: a new frame holding the identity (all ones / zero);  FOLD_AND / FOLD_OR: pop v, top &= / |= v.  An AND without children is
// true, an OR without children false.  Conditions are stored grouped by column, so a column's arrays are read once per group of rows
// however many conditions name it.
//
// Limits, chosen so that the program travels as one by-value kernel argument (MetaProgram is ~1.3 KiB) and sets / bitsets as one
// device block: MP_MAX_CONDS conditions, MP_MAX_GROUPS AND / OR nodes, nesting depth MP_MAX_DEPTH, MP_MAX_COLS distinct fields,
// MP_MAX_WORDS 32-bit words of number sets and bitsets (4 MiB: one bitset over 33 million distinct strings).
#pragma once
#include "../../include/leann_backend.h"
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define MP_HD __host__ __device__
#else
#define MP_HD
#endif

#define MP_MAX_CONDS 32
#define MP_MAX_GROUPS 32
#define MP_MAX_DEPTH 8
#define MP_MAX_COLS 8
#define MP_MAX_WORDS (1u << 20)
#define MP_MAX_INSTR (MP_MAX_CONDS + 2 * MP_MAX_GROUPS)

enum { MP_NUM_NEVER = 0, MP_NUM_LT, MP_NUM_LE, MP_NUM_GT, MP_NUM_GE, MP_NUM_EQ, MP_NUM_NE, MP_NUM_IN, MP_NUM_NOT_IN };
enum { MP_STR_NEVER = 0, MP_STR_RANGE, MP_STR_NOT_RANGE, MP_STR_BITSET, MP_STR_NOT_BITSET };
enum { MP_COND_AND = 0, MP_COND_OR, MP_PUSH_AND, MP_PUSH_OR, MP_FOLD_AND, MP_FOLD_OR };
enum { MP_TAGS_PRESENT = 0x7E, MP_TAGS_ALL = 0x7F };

struct MetaCond {
    double c;                   // MP_NUM_LT .. MP_NUM_NE
    uint32_t set_off, set_cnt;  // MP_NUM_IN / NOT_IN: set_cnt doubles at words[set_off] (set_off is even)
    uint32_t str_a, str_b;      // RANGE: [str_a, str_b); BITSET: the bitset starts at words[str_a]
    uint8_t col, tag_mask, num_op, str_op; // col: slot in MetaProgram::col_id
    uint32_t pad_;
};
struct MetaProgram {
    uint32_t n_cond, n_instr, n_cols, depth; // depth: frames the stack needs, the answer's included
    uint16_t col_id[MP_MAX_COLS];            // the store's column behind each slot
    uint8_t col_first[MP_MAX_COLS + 1];      // conditions [col_first[s], col_first[s + 1]) test slot s
    uint8_t col_need[MP_MAX_COLS];           // bit 0: some condition has a num_test, bit 1: a str_test
    MetaCond cond[MP_MAX_CONDS];
    uint16_t instr[MP_MAX_INSTR];            // op << 8 | condition
};

// the two row tests, the same code on the host and in the kernel
MP_HD inline bool meta_num_eq(double x, double c) { return fabs(x - c) < DBL_EPSILON; } // values_equal, filter.rs:393-395
MP_HD inline bool meta_num_test(const MetaCond &k, const uint32_t *words, double x) {
    switch (k.num_op) {
    case MP_NUM_LT: return x < k.c;
    case MP_NUM_LE: return x <= k.c;
    case MP_NUM_GT: return x > k.c;
    case MP_NUM_GE: return x >= k.c;
    case MP_NUM_EQ: return meta_num_eq(x, k.c);
    case MP_NUM_NE: return !meta_num_eq(x, k.c);
    case MP_NUM_IN:
    case MP_NUM_NOT_IN: {
        const double *set = reinterpret_cast<const double *>(words + k.set_off);
        bool in = false;
        for (uint32_t i = 0; i < k.set_cnt; i++) in = in || meta_num_eq(x, set[i]);
        return in == (k.num_op == MP_NUM_IN);
    }
    default: return false;
    }
}
MP_HD inline bool meta_str_test(const MetaCond &k, const uint32_t *words, uint32_t code) {
    switch (k.str_op) {
    case MP_STR_RANGE: return code >= k.str_a && code < k.str_b;
    case MP_STR_NOT_RANGE: return !(code >= k.str_a && code < k.str_b);
    case MP_STR_BITSET: return (words[k.str_a + (code >> 5)] >> (code & 31)) & 1u;
    case MP_STR_NOT_BITSET: return !((words[k.str_a + (code >> 5)] >> (code & 31)) & 1u);
    default: return false;
    }
}
MP_HD inline bool meta_cond_test(const MetaCond &k, const uint32_t *words, uint32_t tag, double num, uint32_t code) {
    bool m = (k.tag_mask >> tag) & 1u;
    if (tag == LEANN_META_NUMBER && k.num_op != MP_NUM_NEVER) m = m || meta_num_test(k, words, num);
    if (tag == LEANN_META_STRING && k.str_op != MP_STR_NEVER) m = m || meta_str_test(k, words, code);
    return m;
}

// A column as the compiler sees it: its field and its dictionary (sorted, distinct).
struct MetaColumnRef {
    std::string field;
    const std::vector<std::string> *dict;
};

namespace meta_plan_detail {
inline uint32_t lb(const std::vector<std::string> &d, const std::string &s) { return (uint32_t)(std::lower_bound(d.begin(), d.end(), s) - d.begin()); }
inline uint32_t ub(const std::vector<std::string> &d, const std::string &s) { return (uint32_t)(std::upper_bound(d.begin(), d.end(), s) - d.begin()); }
inline bool ends_with(const std::string &s, const std::string &p) { return s.size() >= p.size() && memcmp(s.data() + s.size() - p.size(), p.data(), p.size()) == 0; }

struct Compiler {
    const leann_meta_node *nodes;
    size_t n_nodes, at = 0, n_groups = 0;
    const std::vector<MetaColumnRef> &columns;
    MetaProgram *P;
    std::vector<uint32_t> *words;
    std::string *err;
    uint32_t max_depth = 0;
    std::vector<uint8_t> cond_slot; // tree order

    bool fail(const std::string &msg) { *err = msg; return false; }
    bool reserve_words(size_t count, uint32_t *off) { // zeroed, at an even offset
        if (words->size() & 1) words->push_back(0);
        if (words->size() + count > MP_MAX_WORDS)
            return fail("metadata filter: more than " + std::to_string(MP_MAX_WORDS) + " words of number sets and dictionary bitsets (the limit)");
        *off = (uint32_t)words->size();
        words->resize(words->size() + count, 0);
        return true;
    }
    // the Eq parts of one scalar value, ORed into what an In list has gathered so far
    void eq_scalar(const leann_meta_value &v, uint8_t *bits, std::vector<double> *nums, std::vector<std::string> *strs) {
        switch (v.type) {
        case LEANN_META_VAL_NULL: *bits |= 1u << LEANN_META_NULL; break;
        case LEANN_META_VAL_BOOL: *bits |= 1u << (v.boolean ? LEANN_META_TRUE : LEANN_META_FALSE); break;
        case LEANN_META_VAL_NUMBER: nums->push_back(v.num); break;
        case LEANN_META_VAL_STRING: strs->push_back(std::string(v.str ? v.str : "", v.str ? v.len : 0)); break;
        default: break; // a list equals nothing
        }
    }
    bool cond(const leann_meta_node &nd, MetaCond *k, uint8_t *slot) {
        if (!nd.field) return fail("metadata filter: a condition without a field");
        if (nd.op < LEANN_META_OP_EQ || nd.op > LEANN_META_OP_EXISTS) return fail("metadata filter: unknown op " + std::to_string(nd.op));
        const leann_meta_value &v = nd.value;
        if (v.type < LEANN_META_VAL_NULL || v.type > LEANN_META_VAL_LIST) return fail("metadata filter: unknown value type " + std::to_string(v.type));
        if (v.type == LEANN_META_VAL_LIST && v.len && !v.list) return fail("metadata filter: a list value without elements");
        size_t ci = 0;
        while (ci < columns.size() && columns[ci].field != nd.field) ci++;
        if (ci == columns.size()) return fail(std::string("metadata filter: no column for field '") + nd.field + "'");
        uint32_t s = 0;
        while (s < P->n_cols && P->col_id[s] != ci) s++;
        if (s == P->n_cols) {
            if (s == MP_MAX_COLS) return fail("metadata filter: more than " + std::to_string(MP_MAX_COLS) + " distinct fields (the limit)");
            P->col_id[P->n_cols++] = (uint16_t)ci;
        }
        *slot = (uint8_t)s;
        const std::vector<std::string> &dict = *columns[ci].dict;
        const uint32_t D = (uint32_t)dict.size();
        memset(k, 0, sizeof *k);
        k->col = (uint8_t)s;
        const bool is_num = v.type == LEANN_META_VAL_NUMBER, is_str = v.type == LEANN_META_VAL_STRING;
        const std::string sv = is_str ? std::string(v.str ? v.str : "", v.str ? v.len : 0) : std::string();
        const uint8_t NB = 1u << LEANN_META_NUMBER, SB = 1u << LEANN_META_STRING;
        switch (nd.op) {
        case LEANN_META_OP_EXISTS: k->tag_mask = MP_TAGS_PRESENT; break;
        case LEANN_META_OP_EQ:
        case LEANN_META_OP_NE:
        case LEANN_META_OP_IN:
        case LEANN_META_OP_NOT_IN: {
            const bool list_op = nd.op == LEANN_META_OP_IN || nd.op == LEANN_META_OP_NOT_IN;
            const bool neg = nd.op == LEANN_META_OP_NE || nd.op == LEANN_META_OP_NOT_IN;
            uint8_t bits = 0;
            std::vector<double> nums;
            std::vector<std::string> strs;
            if (!list_op) eq_scalar(v, &bits, &nums, &strs);
            else if (v.type == LEANN_META_VAL_LIST)
                for (size_t i = 0; i < v.len; i++) {
                    if (v.list[i].type < LEANN_META_VAL_NULL || v.list[i].type > LEANN_META_VAL_LIST)
                        return fail("metadata filter: unknown value type " + std::to_string(v.list[i].type) + " in a list");
                    eq_scalar(v.list[i], &bits, &nums, &strs);
                }
            // (In with a value that is no list: nothing matches; NotIn: everything does — the empty gathering says both)
            if (nums.size() == 1 && !list_op) { k->num_op = neg ? MP_NUM_NE : MP_NUM_EQ; k->c = nums[0]; }
            else if (!nums.empty()) {
                if (!reserve_words(2 * nums.size(), &k->set_off)) return false;
                memcpy(words->data() + k->set_off, nums.data(), 8 * nums.size());
                k->set_cnt = (uint32_t)nums.size();
                k->num_op = neg ? MP_NUM_NOT_IN : MP_NUM_IN;
            }
            if (strs.size() == 1) { k->str_op = neg ? MP_STR_NOT_RANGE : MP_STR_RANGE; k->str_a = lb(dict, strs[0]); k->str_b = ub(dict, strs[0]); }
            else if (!strs.empty()) {
                if (!reserve_words(((size_t)D + 31) / 32 + 1, &k->str_a)) return false; // (+ 1: an empty dictionary still has a word)
                for (const std::string &x : strs) {
                    const uint32_t a = lb(dict, x);
                    if (a < ub(dict, x)) (*words)[k->str_a + (a >> 5)] |= 1u << (a & 31);
                }
                k->str_op = neg ? MP_STR_NOT_BITSET : MP_STR_BITSET;
            }
            k->tag_mask = bits;
            if (neg) k->tag_mask = (uint8_t)(MP_TAGS_ALL & ~bits & ~(k->num_op ? NB : 0) & ~(k->str_op ? SB : 0));
            break;
        }
        case LEANN_META_OP_GT:
        case LEANN_META_OP_GTE:
        case LEANN_META_OP_LT:
        case LEANN_META_OP_LTE: {
            const bool incl = nd.op == LEANN_META_OP_GTE || nd.op == LEANN_META_OP_LTE, up = nd.op == LEANN_META_OP_GT || nd.op == LEANN_META_OP_GTE;
            k->tag_mask = incl ? MP_TAGS_PRESENT : 0; // compare_values == 0 for every pair that is not number / number or string / string
            if (is_num) {
                k->tag_mask &= (uint8_t)~NB;
                k->num_op = up ? (incl ? MP_NUM_GE : MP_NUM_GT) : (incl ? MP_NUM_LE : MP_NUM_LT);
                k->c = v.num;
            } else if (is_str) {
                k->tag_mask &= (uint8_t)~SB;
                k->str_op = MP_STR_RANGE;
                if (up) { k->str_a = incl ? lb(dict, sv) : ub(dict, sv); k->str_b = D; }
                else { k->str_a = 0; k->str_b = incl ? ub(dict, sv) : lb(dict, sv); }
            }
            break;
        }
        case LEANN_META_OP_STARTS_WITH: {
            std::string succ = sv; // "" for a value that is no string
            while (!succ.empty() && (unsigned char)succ.back() == 0xFF) succ.pop_back();
            k->str_op = MP_STR_RANGE;
            k->str_a = lb(dict, sv);
            if (succ.empty()) k->str_b = D;
            else { succ.back() = (char)((unsigned char)succ.back() + 1); k->str_b = lb(dict, succ); }
            break;
        }
        default: { // Contains / EndsWith
            if (sv.empty()) { k->str_op = MP_STR_RANGE; k->str_a = 0; k->str_b = D; break; }
            if (!reserve_words(((size_t)D + 31) / 32 + 1, &k->str_a)) return false;
            for (uint32_t i = 0; i < D; i++) {
                const bool hit = nd.op == LEANN_META_OP_CONTAINS ? dict[i].find(sv) != std::string::npos : ends_with(dict[i], sv);
                if (hit) (*words)[k->str_a + (i >> 5)] |= 1u << (i & 31);
            }
            k->str_op = MP_STR_BITSET;
            break;
        }
        }
        return true;
    }
    bool emit(uint32_t op, uint32_t arg) {
        P->instr[P->n_instr++] = (uint16_t)(op << 8 | arg); // (n_instr <= MP_MAX_CONDS + 2 MP_MAX_GROUPS by the two counts below)
        return true;
    }
    bool node(int parent_kind, uint32_t depth) { // depth: AND / OR nodes around this one
        if (at >= n_nodes) return fail("metadata filter: the tree ends before its last node (child counts exceed n_nodes)");
        const leann_meta_node &nd = nodes[at++];
        const bool under_and = parent_kind == LEANN_META_AND;
        if (nd.kind == LEANN_META_COND) {
            if (P->n_cond == MP_MAX_CONDS) return fail("metadata filter: more than " + std::to_string(MP_MAX_CONDS) + " conditions (the limit)");
            uint8_t slot = 0;
            if (!cond(nd, &P->cond[P->n_cond], &slot)) return false;
            cond_slot.push_back(slot);
            return emit(under_and ? MP_COND_AND : MP_COND_OR, P->n_cond++);
        }
        if (nd.kind != LEANN_META_AND && nd.kind != LEANN_META_OR) return fail("metadata filter: unknown node kind " + std::to_string(nd.kind));
        if (depth == MP_MAX_DEPTH) return fail("metadata filter: nested deeper than " + std::to_string(MP_MAX_DEPTH) + " AND / OR levels (the limit)");
        if (n_groups == MP_MAX_GROUPS) return fail("metadata filter: more than " + std::to_string(MP_MAX_GROUPS) + " AND / OR nodes (the limit)");
        n_groups++;
        max_depth = std::max(max_depth, depth + 1);
        emit(nd.kind == LEANN_META_AND ? MP_PUSH_AND : MP_PUSH_OR, 0);
        for (uint32_t c = 0; c < nd.n_children; c++)
            if (!node(nd.kind, depth + 1)) return false;
        return emit(under_and ? MP_FOLD_AND : MP_FOLD_OR, 0);
    }
};
} // namespace meta_plan_detail

// nodes [n_nodes]: the tree in prefix order.  LEANN_OK, or LEANN_ERR_INVALID with *err naming what was wrong; *P and *words are then
// unspecified.  words: number sets and bitsets, for the device as they are.
inline int meta_compile(const leann_meta_node *nodes, size_t n_nodes, const std::vector<MetaColumnRef> &columns, MetaProgram *P,
                        std::vector<uint32_t> *words, std::string *err) {
    memset(P, 0, sizeof *P);
    words->clear();
    if (!nodes || !n_nodes) { *err = "metadata filter: no nodes"; return LEANN_ERR_INVALID; }
    meta_plan_detail::Compiler c{nodes, n_nodes, 0, 0, columns, P, words, err, 0, {}};
    if (!c.node(LEANN_META_OR, 0)) return LEANN_ERR_INVALID;
    if (c.at != n_nodes) { *err = "metadata filter: " + std::to_string(n_nodes - c.at) + " nodes behind the end of the tree"; return LEANN_ERR_INVALID; }
    P->depth = c.max_depth + 1;
    // group the conditions by column slot (stable), and point the instructions at their new places
    uint8_t where[MP_MAX_CONDS];
    MetaCond sorted[MP_MAX_CONDS];
    uint32_t k = 0;
    for (uint32_t s = 0; s < P->n_cols; s++) {
        P->col_first[s] = (uint8_t)k;
        for (uint32_t i = 0; i < P->n_cond; i++)
            if (c.cond_slot[i] == s) {
                if (P->cond[i].num_op) P->col_need[s] |= 1;
                if (P->cond[i].str_op) P->col_need[s] |= 2;
                where[i] = (uint8_t)k;
                sorted[k++] = P->cond[i];
            }
    }
    for (uint32_t s = P->n_cols; s <= MP_MAX_COLS; s++) P->col_first[s] = (uint8_t)k;
    for (uint32_t i = 0; i < P->n_cond; i++) P->cond[i] = sorted[i];
    for (uint32_t i = 0; i < P->n_instr; i++)
        if ((P->instr[i] >> 8) <= MP_COND_OR) P->instr[i] = (uint16_t)((P->instr[i] & 0xFF00) | where[P->instr[i] & 0xFF]);
    if (words->size() & 1) words->push_back(0);
    return LEANN_OK;
}

// The stack program over masks of any width: the kernel runs it on 64-row ballots, the interpreter below on one row.
// cond_mask(i): the mask of condition i.  `stack` holds P.depth entries.
template <typename Mask, typename CondMask>
MP_HD inline Mask meta_run_program(const MetaProgram &P, Mask *stack, CondMask cond_mask) {
    uint32_t sp = 0;
    stack[0] = 0;
    for (uint32_t i = 0; i < P.n_instr; i++) {
        const uint32_t op = P.instr[i] >> 8, arg = P.instr[i] & 0xFF;
        switch (op) {
        case MP_COND_AND: stack[sp] &= cond_mask(arg); break;
        case MP_COND_OR: stack[sp] |= cond_mask(arg); break;
        case MP_PUSH_AND: stack[++sp] = ~(Mask)0; break;
        case MP_PUSH_OR: stack[++sp] = 0; break;
        case MP_FOLD_AND: sp--; stack[sp] &= stack[sp + 1]; break;
        default: sp--; stack[sp] |= stack[sp + 1]; break;
        }
    }
    return stack[0];
}

// One row, on the host: tag / num / code [slot] are the row's entries in the columns of P.col_id.
inline bool meta_eval_row(const MetaProgram &P, const uint32_t *words, const uint8_t *tag, const double *num, const uint32_t *code) {
    uint8_t stack[MP_MAX_DEPTH + 1];
    return meta_run_program<uint8_t>(P, stack, [&](uint32_t i) -> uint8_t {
        const MetaCond &k = P.cond[i];
        return meta_cond_test(k, words, tag[k.col], num[k.col], code[k.col]) ? 0xFF : 0;
    }) & 1;
}
