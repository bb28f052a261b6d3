// meta_batch_selftest — the batch planner of csrc/meta_batch_plan.h on the CPU: no GPU, no library.  Built under AddressSanitizer +
// UBSan.  Reads columns and filter trees from stdin in meta_plan_selftest's format (see there), plus the command `batch`: the filters
// read since the last `batch` (or `n`) are planned as ONE batch against the columns' dictionaries, every launch of the plan is run
// over the rows with the header's scalar interpreter — union columns, remapped programs, relocated words — and printed:
//     plan LAUNCHES N_DISTINCT  then per launch: PROGRAMS/UNION_COLUMNS/WORDS/PAIRS
//     ok <bitmap hex, ceil(n / 8) bytes>        one line per filter of the batch, in batch order
//   or the single line "err <message>" when the planner refuses the batch.
// tests/test_cpu_meta_batch.py compares the bitmaps with a restatement of the reference's filter.rs.
#include "../csrc/meta_batch_plan.h"
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

// what the trees' pointers point at, for the lifetime of a batch
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

static void run_batch(const std::vector<leann_meta_node> &nodes, const std::vector<size_t> &node_off,
                      const std::vector<std::unique_ptr<Column>> &cols, size_t n) {
    std::vector<MetaColumnRef> refs;
    for (const auto &c : cols) refs.push_back(MetaColumnRef{c->field, &c->dict});
    const size_t n_out = node_off.size() - 1;
    MetaBatchPlan plan;
    std::string err;
    if (meta_batch_plan(nodes.data(), node_off.data(), n_out, refs, &plan, &err) != LEANN_OK) {
        printf("err %s\n", err.c_str());
        return;
    }
    printf("plan %zu %zu", plan.launches.size(), plan.n_distinct);
    for (const MetaBatchLaunch &L : plan.launches) printf(" %zu/%zu/%zu/%zu", L.programs.size(), L.cols.size(), L.words.size(), L.pairs.size());
    printf("\n");
    std::vector<std::vector<uint8_t>> bitmaps(n_out, std::vector<uint8_t>((n + 7) / 8, 0));
    std::vector<int> written(n_out, 0);
    for (const MetaBatchLaunch &L : plan.launches) {
        if (L.programs.size() > MB_MAX_PROGRAMS || L.cols.size() > MB_MAX_COLS || L.words.size() > MP_MAX_WORDS) {
            printf("err a launch exceeds a cap\n");
            return;
        }
        std::vector<uint8_t> answer(L.programs.size());
        for (size_t i = 0; i < n; i++) {
            uint8_t tag[MB_MAX_COLS];
            double num[MB_MAX_COLS];
            uint32_t code[MB_MAX_COLS];
            for (size_t u = 0; u < L.cols.size(); u++) {
                const Column &c = *cols[L.cols[u]];
                tag[u] = c.tag[i]; num[u] = c.num[i]; code[u] = c.code[i];
            }
            for (size_t p = 0; p < L.programs.size(); p++) answer[p] = meta_batch_eval_row(L, (uint32_t)p, tag, num, code);
            for (const MetaBatchPair &pr : L.pairs)
                if (answer[pr.prog]) bitmaps[pr.out][i >> 3] |= (uint8_t)(1u << (i & 7));
        }
        for (const MetaBatchPair &pr : L.pairs) written[pr.out]++;
    }
    for (size_t o = 0; o < n_out; o++) {
        if (written[o] != 1) { printf("err output %zu is written by %d pairs\n", o, written[o]); continue; }
        std::string out = "ok ";
        char b[3];
        for (uint8_t x : bitmaps[o]) { snprintf(b, sizeof b, "%02x", x); out += b; }
        puts(out.c_str());
    }
}

int main() {
    std::vector<std::unique_ptr<Column>> cols;
    size_t n = 0;
    std::unique_ptr<Arena> ar(new Arena());
    std::vector<leann_meta_node> nodes;
    std::vector<size_t> node_off{0};
    auto forget = [&] { nodes.clear(); node_off.assign(1, 0); ar.reset(new Arena()); };
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "n") { std::cin >> n; cols.clear(); forget(); }
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
            for (size_t i = 0; i < k; i++) {
                std::string kind, f;
                std::cin >> kind;
                leann_meta_node nd{};
                if (kind == "C") {
                    int op = 0;
                    std::cin >> f >> op;
                    ar->strings.push_back(unhex(f));
                    nd.kind = LEANN_META_COND; nd.field = ar->strings.back().c_str(); nd.op = op; nd.value = read_value(std::cin, *ar);
                } else {
                    uint32_t ch = 0;
                    std::cin >> ch;
                    nd.kind = kind == "A" ? LEANN_META_AND : LEANN_META_OR; nd.n_children = ch;
                }
                nodes.push_back(nd);
            }
            node_off.push_back(nodes.size());
        } else if (cmd == "batch") {
            run_batch(nodes, node_off, cols, n);
            forget();
        } else {
            fprintf(stderr, "meta_batch_selftest: unknown command '%s'\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
