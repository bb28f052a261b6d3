// meta_plan_selftest — the filter compiler of csrc/meta_plan.h on the CPU: no GPU, no library.  Built under AddressSanitizer + UBSan.
// Reads columns and filter trees from stdin, compiles each tree against the columns' dictionaries, runs the compiled program over the
// rows with the header's scalar interpreter and prints the bitmap; tests/test_cpu_meta_plan.py compares it with a restatement of the
// reference's filter.rs.  Whitespace-separated tokens; strings are hex ("-" = empty), numbers the hex of their 64 bits:
//     n ROWS
//     column FIELD D  dict[0] .. dict[D-1]  then per row: TAG NUM CODE
//     filter N_NODES  then per node, prefix order:  C FIELD OP VALUE | A CHILDREN | O CHILDREN
//         VALUE: n | b 0|1 | f BITS | s HEX | l COUNT VALUE...
//   -> one line per filter: "ok <bitmap hex, ceil(n / 8) bytes>" or "err <message>"
// --limits: every limit of the header one past it, and at it; prints "name rc message" lines.
#include "../csrc/meta_plan.h"
#include <cstdio>
#include <deque>
#include <iostream>
#include <memory>

struct Column {
    std::string field;
    std::vector<std::string> dict;
    std::vector<uint8_t> tag;
    std::vector<double> num;
    std::vector<uint32_t> code;
};

static std::string unhex(const std::string &h) {
    std::string s;
    if (h == "-") return s;
    for (size_t i = 0; i + 1 < h.size(); i += 2) s.push_back((char)std::stoi(h.substr(i, 2), nullptr, 16));
    return s;
}
static double bits_f64(const std::string &h) {
    const uint64_t b = std::stoull(h, nullptr, 16);
    double d;
    memcpy(&d, &b, 8);
    return d;
}

// what a tree's pointers point at
struct Arena {
    std::deque<std::string> strings;
    std::deque<std::vector<leann_meta_value>> lists;
};
static leann_meta_value read_value(std::istream &in, Arena &ar, bool in_list = false) {
    leann_meta_value v{};
    std::string t, x;
    in >> t;
    if (t == "n") v.type = LEANN_META_VAL_NULL;
    else if (t == "b") { in >> x; v.type = LEANN_META_VAL_BOOL; v.boolean = x == "1"; }
    else if (t == "f") { in >> x; v.type = LEANN_META_VAL_NUMBER; v.num = bits_f64(x); }
    else if (t == "s") {
        in >> x;
        ar.strings.push_back(unhex(x));
        v.type = LEANN_META_VAL_STRING;
        v.str = ar.strings.back().data();
        v.len = ar.strings.back().size();
    } else if (t == "l" && !in_list) {
        size_t cnt = 0;
        in >> cnt;
        ar.lists.emplace_back();
        std::vector<leann_meta_value> &l = ar.lists.back();
        for (size_t i = 0; i < cnt; i++) l.push_back(read_value(in, ar, true));
        v.type = LEANN_META_VAL_LIST;
        v.len = cnt;
        v.list = l.data();
    } else v.type = 99;
    return v;
}

static std::string run(const std::vector<leann_meta_node> &nodes, const std::vector<std::unique_ptr<Column>> &cols, size_t n) {
    std::vector<MetaColumnRef> refs;
    for (const auto &c : cols) refs.push_back(MetaColumnRef{c->field, &c->dict});
    MetaProgram P;
    std::vector<uint32_t> words;
    std::string err;
    if (meta_compile(nodes.data(), nodes.size(), refs, &P, &words, &err) != LEANN_OK) return "err " + err;
    std::vector<uint8_t> bitmap((n + 7) / 8, 0);
    for (size_t i = 0; i < n; i++) {
        uint8_t tag[MP_MAX_COLS];
        double num[MP_MAX_COLS];
        uint32_t code[MP_MAX_COLS];
        for (uint32_t s = 0; s < P.n_cols; s++) {
            const Column &c = *cols[P.col_id[s]];
            tag[s] = c.tag[i]; num[s] = c.num[i]; code[s] = c.code[i];
        }
        if (meta_eval_row(P, words.data(), tag, num, code)) bitmap[i >> 3] |= (uint8_t)(1u << (i & 7));
    }
    std::string out = "ok ";
    char b[3];
    for (uint8_t x : bitmap) { snprintf(b, sizeof b, "%02x", x); out += b; }
    return out;
}

static leann_meta_node cond_node(const char *field, int op, leann_meta_value v) {
    leann_meta_node nd{};
    nd.kind = LEANN_META_COND; nd.field = field; nd.op = op; nd.value = v;
    return nd;
}
static leann_meta_node group_node(int kind, uint32_t children) {
    leann_meta_node nd{};
    nd.kind = kind; nd.n_children = children;
    return nd;
}

static int limits() {
    // one column per field name f0 .. f8; f0 has a dictionary of 2^20 strings ("%07x"): a bitset over it takes 32768 + 1 words
    std::vector<std::unique_ptr<Column>> cols;
    std::vector<std::string> names;
    for (int i = 0; i < 9; i++) {
        cols.emplace_back(new Column());
        cols.back()->field = "f" + std::to_string(i);
        names.push_back(cols.back()->field);
    }
    char buf[16];
    for (uint32_t i = 0; i < (1u << 20); i++) { snprintf(buf, sizeof buf, "%07x", i); cols[0]->dict.emplace_back(buf); }
    leann_meta_value num{};
    num.type = LEANN_META_VAL_NUMBER; num.num = 1.0;
    leann_meta_value pat{};
    pat.type = LEANN_META_VAL_STRING; pat.str = "a"; pat.len = 1;
    auto report = [&](const char *name, const std::vector<leann_meta_node> &nodes) {
        const std::string r = run(nodes, cols, 0);
        printf("%s %d %s\n", name, r.compare(0, 3, "err") == 0 ? LEANN_ERR_INVALID : LEANN_OK, r.c_str() + (r.size() > 3 ? 3 : r.size()));
    };
    for (uint32_t k : {(uint32_t)MP_MAX_CONDS, (uint32_t)MP_MAX_CONDS + 1}) { // conditions
        std::vector<leann_meta_node> t{group_node(LEANN_META_AND, k)};
        for (uint32_t i = 0; i < k; i++) t.push_back(cond_node("f1", LEANN_META_OP_GT, num));
        report(k == MP_MAX_CONDS ? "conds_at" : "conds_past", t);
    }
    for (uint32_t d : {(uint32_t)MP_MAX_DEPTH, (uint32_t)MP_MAX_DEPTH + 1}) { // nesting
        std::vector<leann_meta_node> t;
        for (uint32_t i = 0; i < d; i++) t.push_back(group_node(i & 1 ? LEANN_META_OR : LEANN_META_AND, 1));
        t.push_back(cond_node("f1", LEANN_META_OP_GT, num));
        report(d == MP_MAX_DEPTH ? "depth_at" : "depth_past", t);
    }
    for (uint32_t g : {(uint32_t)MP_MAX_GROUPS, (uint32_t)MP_MAX_GROUPS + 1}) { // AND / OR nodes: a root with g - 1 empty groups below it
        std::vector<leann_meta_node> t{group_node(LEANN_META_OR, g - 1)};
        for (uint32_t i = 0; i + 1 < g; i++) t.push_back(group_node(LEANN_META_AND, 0));
        report(g == MP_MAX_GROUPS ? "groups_at" : "groups_past", t);
    }
    for (uint32_t c : {(uint32_t)MP_MAX_COLS, (uint32_t)MP_MAX_COLS + 1}) { // distinct fields
        std::vector<leann_meta_node> t{group_node(LEANN_META_AND, c)};
        for (uint32_t i = 0; i < c; i++) t.push_back(cond_node(names[i].c_str(), LEANN_META_OP_GT, num));
        report(c == MP_MAX_COLS ? "cols_at" : "cols_past", t);
    }
    { // words: 31 bitsets of 32769 words, each at an even offset (32770 apart), leave 2^20 - 31 * 32770 = 32706 words: a set of 16353
      // numbers fills them exactly, one more is one past the limit
        const uint32_t left = MP_MAX_WORDS - 31u * 32770u;
        for (uint32_t extra : {0u, 1u}) {
            std::vector<leann_meta_value> set(left / 2 + extra, num);
            leann_meta_value lst{};
            lst.type = LEANN_META_VAL_LIST; lst.len = set.size(); lst.list = set.data();
            std::vector<leann_meta_node> t{group_node(LEANN_META_OR, 32)};
            for (int i = 0; i < 31; i++) t.push_back(cond_node("f0", LEANN_META_OP_CONTAINS, pat));
            t.push_back(cond_node("f1", LEANN_META_OP_IN, lst));
            report(extra ? "words_past" : "words_at", t);
        }
    }
    report("no_column", {cond_node("nowhere.at.all", LEANN_META_OP_EXISTS, num)});
    report("short_tree", {group_node(LEANN_META_AND, 2), cond_node("f1", LEANN_META_OP_GT, num)});
    report("long_tree", {cond_node("f1", LEANN_META_OP_GT, num), cond_node("f1", LEANN_META_OP_GT, num)});
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && std::string(argv[1]) == "--limits") return limits();
    std::vector<std::unique_ptr<Column>> cols;
    size_t n = 0;
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "n") { std::cin >> n; cols.clear(); }
        else if (cmd == "column") {
            std::string f, x;
            size_t D = 0;
            std::cin >> f >> D;
            std::unique_ptr<Column> c(new Column());
            c->field = unhex(f);
            for (size_t i = 0; i < D; i++) { std::cin >> x; c->dict.push_back(unhex(x)); }
            for (size_t i = 0; i < n; i++) {
                unsigned tag = 0;
                uint32_t code = 0;
                std::cin >> tag >> x >> code;
                c->tag.push_back((uint8_t)tag); c->num.push_back(bits_f64(x)); c->code.push_back(code);
            }
            cols.push_back(std::move(c));
        } else if (cmd == "filter") {
            size_t k = 0;
            std::cin >> k;
            Arena ar;
            std::vector<leann_meta_node> nodes;
            for (size_t i = 0; i < k; i++) {
                std::string kind, f;
                std::cin >> kind;
                if (kind == "C") {
                    int op = 0;
                    std::cin >> f >> op;
                    ar.strings.push_back(unhex(f));
                    const char *field = ar.strings.back().c_str();
                    nodes.push_back(cond_node(field, op, read_value(std::cin, ar)));
                } else {
                    uint32_t ch = 0;
                    std::cin >> ch;
                    nodes.push_back(group_node(kind == "A" ? LEANN_META_AND : LEANN_META_OR, ch));
                }
            }
            puts(run(nodes, cols, n).c_str());
        } else {
            fprintf(stderr, "meta_plan_selftest: unknown command '%s'\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
