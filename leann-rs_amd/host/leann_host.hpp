// leann_host.hpp — C++ host-side mirror of leann-rs's index layer above the C ABI
// (the reference is Rust; no Rust toolchain exists in this image).
// Same names, argument meaning and error behaviour as the reference for the path:
//     IndexMeta            src/index/meta.rs:9-58
//     PassageStore         src/index/passages.rs:11-105
//     tokenize / Bm25Scorer / hybrid_rerank   src/index/bm25.rs:9-170   (f32, op for op)
//     MetadataFilter       src/index/filter.rs (mini-language evaluated on passage metadata)
//     find_index           src/index/locate.rs:11-36
//     SearchOptions / SearchResult / IndexSearcher   src/index/searcher.rs:15-257
//     RecomputeSearcher    src/index/recompute.rs:17-139   (arithmetic on the GPU: leann_scan_topk_device)
// Vector search itself always goes through include/leann_backend.h (HIP kernels); nothing here
// computes distances on the CPU.
#pragma once
#include "../../include/leann_backend.h"
#include "json.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fstream>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <optional>
#include <set>
#include <sstream>
#include <stdexcept>
#include <string>
#include <sys/stat.h>
#include <unordered_map>
#include <unordered_set>
#include <vector>

namespace leann {

struct Error : std::runtime_error { using std::runtime_error::runtime_error; };
inline void check(int rc) { if (rc != 0) throw Error(leann_last_error()); }

inline bool file_exists(const std::string &p) { struct stat st; return ::stat(p.c_str(), &st) == 0; }
inline std::string read_file(const std::string &p) {
    std::ifstream f(p, std::ios::binary);
    if (!f) throw Error("No such file or directory: " + p);
    std::stringstream ss;
    ss << f.rdbuf();
    return ss.str();
}
// Path::with_extension on ".../documents.leann": replace the text after the last '.' of the file name
inline std::string with_extension(const std::string &stem, const std::string &ext) {
    size_t slash = stem.find_last_of('/'), dot = stem.find_last_of('.');
    bool has = dot != std::string::npos && (slash == std::string::npos || dot > slash + 1);
    return (has ? stem.substr(0, dot) : stem) + "." + ext;
}

// ---- src/index/meta.rs ---------------------------------------------------------------------------
struct IndexMeta {
    std::string version, backend_name, embedding_model, embedding_mode;
    size_t dimensions = 0, passage_count = 0;
    lj::Value backend_kwargs, embedding_options; // optional
    bool is_recompute = false, is_pruned = false;

    static IndexMeta load(const std::string &path) {
        lj::Value v = lj::parse(read_file(path));
        auto need = [&](const char *k) -> const lj::Value & {
            const lj::Value *x = v.get(k);
            if (!x) throw Error(std::string("missing field `") + k + "`");
            return *x;
        };
        IndexMeta m;
        m.version = need("version").s;
        m.backend_name = need("backend_name").s;
        m.embedding_model = need("embedding_model").s;
        m.embedding_mode = need("embedding_mode").s;
        m.dimensions = (size_t)need("dimensions").as_f64();
        m.passage_count = (size_t)need("passage_count").as_f64();
        if (auto *x = v.get("backend_kwargs")) m.backend_kwargs = *x;
        if (auto *x = v.get("embedding_options")) m.embedding_options = *x;
        if (auto *x = v.get("is_recompute")) m.is_recompute = x->b;   // #[serde(default)]
        if (auto *x = v.get("is_pruned")) m.is_pruned = x->b;
        return m;
    }
    void save(const std::string &path) const {
        lj::Value v = lj::Value::object();
        v["version"] = lj::Value::string(version);
        v["backend_name"] = lj::Value::string(backend_name);
        v["embedding_model"] = lj::Value::string(embedding_model);
        v["embedding_mode"] = lj::Value::string(embedding_mode);
        v["dimensions"] = lj::Value::integer((int64_t)dimensions);
        v["passage_count"] = lj::Value::integer((int64_t)passage_count);
        if (!backend_kwargs.is_null()) v["backend_kwargs"] = backend_kwargs; // skip_serializing_if None
        if (!embedding_options.is_null()) v["embedding_options"] = embedding_options;
        v["is_recompute"] = lj::Value::boolean(is_recompute);
        v["is_pruned"] = lj::Value::boolean(is_pruned);
        std::ofstream(path) << lj::to_string_pretty(v);
    }
};

// ---- src/index/passages.rs -------------------------------------------------------------------------
struct Passage {
    std::string id, text;
    lj::Value metadata;
};
class PassageStore {
  public:
    static PassageStore open(const std::string &base_path) {
        PassageStore s;
        s.jsonl_path_ = with_extension(base_path, "passages.jsonl");
        lj::Value idx = lj::parse(read_file(with_extension(base_path, "passages.idx.json")));
        if (!idx.is_object()) throw Error("passages.idx.json: expected an object");
        for (auto &kv : *idx.o) s.offsets_[kv.first] = (uint64_t)kv.second.as_f64();
        return s;
    }
    Passage get(const std::string &id) const { // one open + seek + one line, like passages.rs:90-105
        auto it = offsets_.find(id);
        if (it == offsets_.end()) throw Error("Passage not found: " + id);
        std::ifstream f(jsonl_path_, std::ios::binary);
        if (!f) throw Error("cannot open " + jsonl_path_);
        f.seekg((std::streamoff)it->second);
        std::string line;
        std::getline(f, line);
        lj::Value v = lj::parse(line);
        Passage p;
        if (auto *x = v.get("id")) p.id = x->s;
        if (auto *x = v.get("text")) p.text = x->s;
        if (auto *x = v.get("metadata")) p.metadata = *x;
        return p;
    }
    std::vector<std::string> ids() const {
        std::vector<std::string> r;
        for (auto &kv : offsets_) r.push_back(kv.first);
        return r;
    }
    size_t len() const { return offsets_.size(); }

  private:
    std::unordered_map<std::string, uint64_t> offsets_;
    std::string jsonl_path_;
};
class PassageStoreWriter { // passages.rs:120-158
  public:
    explicit PassageStoreWriter(const std::string &base_path)
        : idx_path_(with_extension(base_path, "passages.idx.json")), out_(with_extension(base_path, "passages.jsonl"), std::ios::binary) {}
    void add(const Passage &p) {
        lj::Value v = lj::Value::object();
        v["id"] = lj::Value::string(p.id);
        v["text"] = lj::Value::string(p.text);
        v["metadata"] = p.metadata;
        std::string line = lj::to_string(v);
        offsets_[p.id] = cur_;
        out_ << line << '\n';
        cur_ += line.size() + 1;
    }
    void finish() {
        out_.flush();
        lj::Value idx = lj::Value::object();
        for (auto &kv : offsets_) idx[kv.first] = lj::Value::integer((int64_t)kv.second);
        std::ofstream(idx_path_) << lj::to_string(idx);
    }

  private:
    std::string idx_path_;
    std::ofstream out_;
    std::map<std::string, uint64_t> offsets_;
    uint64_t cur_ = 0;
};

// ---- src/index/bm25.rs -----------------------------------------------------------------------------
inline std::vector<std::string> tokenize(const std::string &text) { // [a-zA-Z0-9]+, lowercase, len > 1
    std::vector<std::string> out;
    std::string cur;
    auto flush = [&] { if (cur.size() > 1) out.push_back(cur); cur.clear(); };
    for (unsigned char c : text) {
        if ((c >= 'a' && c <= 'z') || (c >= '0' && c <= '9')) cur += (char)c;
        else if (c >= 'A' && c <= 'Z') cur += (char)(c - 'A' + 'a');
        else flush();
    }
    flush();
    return out;
}

class Bm25Scorer {
  public:
    static constexpr float K1 = 1.2f, B = 0.75f; // bm25.rs:9-10
    // bm25.rs:33-74.  The reference keeps one term -> tf map per passage and probes every one of them per query token; here the same
    // counts are kept inverted — a term dictionary and, per term, its (passage, tf) postings in ascending passage order — built in the
    // same single pass.  doc_freq of a term is the length of its list.
    static Bm25Scorer build(const std::vector<std::string> &documents) {
        Bm25Scorer s;
        s.num_docs_ = documents.size();
        size_t total = 0;
        for (size_t doc = 0; doc < documents.size(); doc++) {
            auto toks = tokenize(documents[doc]);
            s.doc_lengths_.push_back(toks.size());
            total += toks.size();
            for (auto &t : toks) {
                auto it = s.term_ids_.find(t);
                if (it == s.term_ids_.end()) {
                    it = s.term_ids_.emplace(t, (uint32_t)s.postings_.size()).first;
                    s.postings_.emplace_back();
                }
                auto &list = s.postings_[it->second];
                if (!list.empty() && list.back().first == (uint32_t)doc) list.back().second++;
                else list.emplace_back((uint32_t)doc, 1u);
            }
        }
        s.avg_doc_len_ = s.num_docs_ > 0 ? (float)total / (float)s.num_docs_ : 1.0f;
        return s;
    }
    float idf(uint32_t term) const {
        float df = (float)postings_[term].size();
        return std::log(((float)num_docs_ - df + 0.5f) / (df + 0.5f) + 1.0f); // :88
    }
    // the query's known tokens in token order (a repeated token twice, bm25.rs:81; unknown ones skipped, :84-86) as (term id, idf)
    std::vector<std::pair<uint32_t, float>> query_terms(const std::string &query) const {
        std::vector<std::pair<uint32_t, float>> out;
        for (auto &token : tokenize(query)) {
            auto it = term_ids_.find(token);
            if (it == term_ids_.end() || postings_[it->second].empty()) continue;
            out.emplace_back(it->second, idf(it->second));
        }
        return out;
    }
    // Walks the posting list of each token instead of probing every passage: per passage the same additions in the same (token) order
    // as bm25.rs:77-106, hence the same bits.
    std::vector<float> score_query(const std::string &query) const {
        std::vector<float> scores(num_docs_, 0.0f);
        for (auto &qt : query_terms(query)) {
            const float idf = qt.second;
            for (auto &p : postings_[qt.first]) {
                const size_t doc = p.first;
                float tf = (float)p.second;
                float doc_len = (float)doc_lengths_[doc];
                float norm = 1.0f - B + B * (doc_len / avg_doc_len_);     // :97
                float score = idf * (tf * (K1 + 1.0f)) / (tf + K1 * norm); // :100
                scores[doc] += score;
            }
        }
        return scores;
    }
    std::vector<std::pair<size_t, float>> search(const std::string &query, size_t top_k) const {
        auto scores = score_query(query);
        std::vector<std::pair<size_t, float>> scored;
        for (size_t i = 0; i < scores.size(); i++)
            if (scores[i] > 0.0f) scored.emplace_back(i, scores[i]);
        std::stable_sort(scored.begin(), scored.end(), [](auto &a, auto &b) { return b.second < a.second; });
        if (scored.size() > top_k) scored.resize(top_k);
        return scored;
    }
    size_t num_docs() const { return num_docs_; }
    size_t num_terms() const { return postings_.size(); }
    float avg_doc_len() const { return avg_doc_len_; }
    const std::unordered_map<std::string, uint32_t> &term_ids() const { return term_ids_; }
    // the inverted index as CSR arrays (leann_bm25_create): post_off [n_terms + 1], post_doc / post_tf, doc_len [n_docs]
    void export_csr(std::vector<uint64_t> &post_off, std::vector<uint32_t> &post_doc, std::vector<uint32_t> &post_tf,
                    std::vector<uint32_t> &doc_len) const {
        post_off.assign(1, 0);
        post_doc.clear();
        post_tf.clear();
        for (auto &list : postings_) {
            for (auto &p : list) { post_doc.push_back(p.first); post_tf.push_back(p.second); }
            post_off.push_back(post_doc.size());
        }
        doc_len.assign(doc_lengths_.begin(), doc_lengths_.end());
    }

  private:
    std::unordered_map<std::string, uint32_t> term_ids_;
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> postings_; // per term: (passage, tf), passages ascending
    size_t num_docs_ = 0;
    float avg_doc_len_ = 1.0f;
    std::vector<size_t> doc_lengths_;
};

// bm25.rs:135-170 — min-max normalise both lists, alpha blend, stable sort descending
// `allow` (additive; include/leann_backend.h "under an allow-bitmap"): min_b / max_b are folded over the positions whose bit is set only
inline std::vector<std::pair<size_t, float>> hybrid_rerank(const std::vector<std::pair<size_t, float>> &vector_results,
                                                           const std::vector<float> &bm25_scores, float alpha,
                                                           const std::vector<uint8_t> *allow = nullptr) {
    float max_v = -INFINITY, min_v = INFINITY;
    for (auto &r : vector_results) { max_v = std::fmax(max_v, r.second); min_v = std::fmin(min_v, r.second); }
    float vrange = std::fmax(max_v - min_v, 1e-6f);
    float max_b = -INFINITY, min_b = INFINITY;
    if (!allow) {
        for (float b : bm25_scores) { max_b = std::fmax(max_b, b); min_b = std::fmin(min_b, b); }
    } else {
        for (size_t i = 0; i < bm25_scores.size() && (i >> 3) < allow->size(); i++)
            if (((*allow)[i >> 3] >> (i & 7)) & 1) { max_b = std::fmax(max_b, bm25_scores[i]); min_b = std::fmin(min_b, bm25_scores[i]); }
    }
    float brange = std::fmax(max_b - min_b, 1e-6f);
    std::vector<std::pair<size_t, float>> out;
    out.reserve(vector_results.size());
    for (auto &r : vector_results) {
        float norm_vec = (r.second - min_v) / vrange;
        float bm = r.first < bm25_scores.size() ? bm25_scores[r.first] : 0.0f;
        float norm_b = (bm - min_b) / brange;
        float t1 = alpha * norm_vec, t2 = (1.0f - alpha) * norm_b;
        out.emplace_back(r.first, t1 + t2);
    }
    std::stable_sort(out.begin(), out.end(), [](auto &a, auto &b) { return b.second < a.second; });
    return out;
}

// ---- src/index/filter.rs (behavioural mirror of the mini-language) -------------------------------------
class MetadataFilter {
  public:
    enum Op { Eq, Ne, Gt, Gte, Lt, Lte, In, NotIn, Contains, StartsWith, EndsWith, Exists };
    static std::optional<MetadataFilter> parse(const std::string &text) {
        std::string s = trim(text);
        if (s.find(" OR ") != std::string::npos) return combine(split(s, " OR "), false, false);
        bool has_and = s.find(" AND ") != std::string::npos;
        if (has_and) return combine(split(s, " AND "), true, true);
        auto parts = split_commas(s);
        if (parts.size() > 1) return combine(parts, true, true);
        return single(s);
    }
    bool matches(const lj::Value &metadata) const {
        if (kind_ == And) { for (auto &c : children_) if (!c.matches(metadata)) return false; return true; }
        if (kind_ == Or) { for (auto &c : children_) if (c.matches(metadata)) return true; return false; }
        const lj::Value *fv = &metadata;
        {
            size_t start = 0;
            for (;;) {
                size_t dot = field_.find('.', start);
                std::string part = field_.substr(start, dot == std::string::npos ? std::string::npos : dot - start);
                fv = fv->get(part);
                if (!fv || dot == std::string::npos) break;
                start = dot + 1;
            }
        }
        auto str_test = [&](auto pred) { return fv && fv->is_string() && value_.is_string() ? pred(fv->s, value_.s) : (fv && fv->is_string() && pred(fv->s, std::string())); };
        switch (op_) {
            case Exists: return fv != nullptr;
            case Eq: return fv && equal(*fv, value_);
            case Ne: return !fv || !equal(*fv, value_);
            case Gt: return fv && compare(*fv, value_) > 0;
            case Gte: return fv && compare(*fv, value_) >= 0;
            case Lt: return fv && compare(*fv, value_) < 0;
            case Lte: return fv && compare(*fv, value_) <= 0;
            case In: if (!fv) return false; for (auto &x : *value_.a) if (equal(*fv, x)) return true; return false;
            case NotIn: if (!fv) return true; for (auto &x : *value_.a) if (equal(*fv, x)) return false; return true;
            case Contains: return str_test([](const std::string &h, const std::string &n) { return h.find(n) != std::string::npos; });
            case StartsWith: return str_test([](const std::string &h, const std::string &n) { return h.compare(0, n.size(), n) == 0; });
            case EndsWith: return str_test([](const std::string &h, const std::string &n) { return h.size() >= n.size() && h.compare(h.size() - n.size(), n.size(), n) == 0; });
        }
        return false;
    }

    // read access to the tree (the device path walks it: IndexSearcher::device_filter)
    bool is_condition() const { return kind_ == Cond; }
    bool is_and() const { return kind_ == And; }
    const std::string &field() const { return field_; }
    Op op() const { return op_; }
    const lj::Value &value() const { return value_; }
    const std::vector<MetadataFilter> &children() const { return children_; }

  private:
    enum Kind { Cond, And, Or } kind_ = Cond;
    std::string field_;
    Op op_ = Eq;
    lj::Value value_;
    std::vector<MetadataFilter> children_;

    static std::string trim(const std::string &s) {
        size_t a = s.find_first_not_of(" \t\n\r"), b = s.find_last_not_of(" \t\n\r");
        return a == std::string::npos ? "" : s.substr(a, b - a + 1);
    }
    static std::vector<std::string> split(const std::string &s, const std::string &sep) {
        std::vector<std::string> out;
        size_t pos = 0, f;
        while ((f = s.find(sep, pos)) != std::string::npos) { out.push_back(s.substr(pos, f - pos)); pos = f + sep.size(); }
        out.push_back(s.substr(pos));
        return out;
    }
    static std::vector<std::string> split_commas(const std::string &s) { // commas outside [...]
        std::vector<std::string> out;
        std::string cur;
        int depth = 0;
        for (char c : s) {
            if (c == '[') depth++;
            if (c == ']') depth--;
            if (c == ',' && depth == 0) { out.push_back(cur); cur.clear(); } else cur += c;
        }
        if (!cur.empty()) out.push_back(cur);
        return out;
    }
    static std::optional<MetadataFilter> combine(const std::vector<std::string> &parts, bool is_and, bool singles) {
        std::vector<MetadataFilter> fs;
        for (auto &p : parts) {
            auto f = singles ? single(trim(p)) : parse(trim(p));
            if (f) fs.push_back(*f);
        }
        if (fs.size() > 1) { MetadataFilter m; m.kind_ = is_and ? And : Or; m.children_ = std::move(fs); return m; }
        if (fs.size() == 1) return fs[0];
        return std::nullopt;
    }
    static lj::Value parse_value(const std::string &s) {
        char *end = nullptr;
        if (!s.empty()) {
            long long iv = strtoll(s.c_str(), &end, 10);
            if (end && *end == 0 && (isdigit((unsigned char)s[0]) || s[0] == '-' || s[0] == '+')) return lj::Value::integer(iv);
            double dv = strtod(s.c_str(), &end);
            if (end && *end == 0 && std::isfinite(dv) && (isdigit((unsigned char)s[0]) || s[0] == '-' || s[0] == '+' || s[0] == '.')) return lj::Value::number(dv);
        }
        if (s == "true") return lj::Value::boolean(true);
        if (s == "false") return lj::Value::boolean(false);
        return lj::Value::string(s);
    }
    static MetadataFilter cond(std::string field, Op op, lj::Value v) {
        MetadataFilter m;
        m.field_ = std::move(field);
        m.op_ = op;
        m.value_ = std::move(v);
        return m;
    }
    static std::optional<MetadataFilter> list_op(const std::string &s, const std::string &kw, Op op) {
        size_t idx = s.find(kw);
        if (idx == std::string::npos) return std::nullopt;
        std::string rest = s.substr(idx + kw.size());
        size_t end = rest.find(']');
        if (end == std::string::npos) return std::nullopt;
        lj::Value arr = lj::Value::array();
        for (auto &v : split(rest.substr(0, end), ",")) arr.a->push_back(parse_value(trim(v)));
        return cond(trim(s.substr(0, idx)), op, arr);
    }
    static std::optional<MetadataFilter> single(const std::string &text) {
        std::string s = trim(text);
        if (s.empty()) return std::nullopt;
        if (s.back() == '?') return cond(s.substr(0, s.size() - 1), Exists, lj::Value());
        if (auto f = list_op(s, " in [", In)) return f;
        if (auto f = list_op(s, " not_in [", NotIn)) return f;
        auto two = [&](const std::string &sep, Op op, bool as_string) -> std::optional<MetadataFilter> {
            size_t p = s.find(sep);
            if (p == std::string::npos) return std::nullopt;
            std::string rhs = s.substr(p + sep.size());
            return cond(s.substr(0, p), op, as_string ? lj::Value::string(rhs) : parse_value(rhs));
        };
        if (s.find('~') != std::string::npos) return two("~", Contains, true);
        if (s.find('^') != std::string::npos && s.find(">=") == std::string::npos) return two("^", StartsWith, true);
        if (s.find('$') != std::string::npos) return two("$", EndsWith, true);
        if (s.find("!=") != std::string::npos) return two("!=", Ne, false);
        if (s.find(">=") != std::string::npos) return two(">=", Gte, false);
        if (s.find("<=") != std::string::npos) return two("<=", Lte, false);
        if (s.find('>') != std::string::npos) return two(">", Gt, false);
        if (s.find('<') != std::string::npos) return two("<", Lt, false);
        size_t p = s.find('=');
        if (p == std::string::npos) p = s.find(':');
        if (p == std::string::npos) return std::nullopt;
        std::string field = s.substr(0, p), value = s.substr(p + 1);
        if (value.find('*') != std::string::npos) { // glob forms
            bool st = value.front() == '*', en = value.back() == '*';
            if (st && en && value.size() > 2) return cond(field, Contains, lj::Value::string(value.substr(1, value.size() - 2)));
            if (st) return cond(field, EndsWith, lj::Value::string(value.substr(1)));
            if (en) return cond(field, StartsWith, lj::Value::string(value.substr(0, value.size() - 1)));
        }
        return cond(field, Eq, parse_value(value));
    }
    static bool equal(const lj::Value &a, const lj::Value &b) {
        if (a.is_string() && b.is_string()) return a.s == b.s;
        if (a.is_number() && b.is_number()) return std::fabs(a.as_f64() - b.as_f64()) < std::numeric_limits<double>::epsilon();
        if (a.kind == lj::Value::Bool && b.kind == lj::Value::Bool) return a.b == b.b;
        return a.is_null() && b.is_null();
    }
    static int compare(const lj::Value &a, const lj::Value &b) {
        if (a.is_number() && b.is_number()) return a.as_f64() < b.as_f64() ? -1 : (a.as_f64() > b.as_f64() ? 1 : 0);
        if (a.is_string() && b.is_string()) return a.s < b.s ? -1 : (a.s > b.s ? 1 : 0);
        return 0;
    }
};

// ---- src/index/locate.rs ---------------------------------------------------------------------------
inline std::string find_index(const std::string &name) {
    std::string local = ".leann/indexes/" + name;
    if (file_exists(local)) return local;
    if (!name.empty() && name[0] == '/' && file_exists(name)) return name;
    if (const char *home = getenv("HOME")) {
        std::string global = std::string(home) + "/.leann/indexes/" + name;
        if (file_exists(global)) return global;
    }
    throw Error("Index '" + name + "' not found. Run 'leann list' to see available indexes.");
}

// ---- src/index/searcher.rs ---------------------------------------------------------------------------
struct SearchResult {
    std::string id;
    float score = 0.f;
    std::string text;
    lj::Value metadata;
};
struct SearchOptions {
    size_t top_k = 5, complexity = 64;
    std::optional<MetadataFilter> filter;
    bool hybrid = false;
    float hybrid_alpha = 0.7f; // searcher.rs:47
    std::optional<std::string> query_text;
    // Additive: evaluate the metadata filter INSIDE the graph traversal (allow-bitmap over
    // positions, leann_backend_search_filtered) instead of over-fetching 5*top_k and post-filtering (:129-133,
    // :190-194).  `filter_key` names the filter for the bitmap cache (the CLI passes the filter text).
    bool device_filter = false;
    std::string filter_key;
    // the reference hands the backend's DISTANCES (1 - dot, lower = better) to hybrid_rerank, which treats a larger
    // vector score as better (bm25.rs:159, sort desc :168) — in hybrid mode the WORST ANN hits rank highest on the vector term.
    // true (default) reproduces that faithfully; false is the corrected mode: the ANN hits enter the blend as similarities 1 - dist
    // (BM25-only hits keep the 0.0 of searcher.rs:160-165).  `leann search --compat-polarity true|false`.
    bool compat_polarity = true;
    // Additive: the BM25 half of hybrid mode runs on the device (leann_bm25, csrc/bm25.hip) when the searcher has a backend and
    // fetch_k <= 256; false — or no device — scores on the host.  Same bits either way.  `leann search --bm25 device|host`.
    bool bm25_device = true;
    // Additive (include/leann_backend.h "under an allow-bitmap"): in hybrid mode the BM25 half sees only the passages the vector half
    // may return — the --device-filter bitmap, or the live positions of an index with removals — so that no BM25-only hit is injected
    // that the post-filter then drops, and a removed or filtered-out best hit does not set max_bm25.  false (default): the filter and
    // the removals act after the rerank, as before.  `leann search --hybrid-filter inside|post`.
    bool hybrid_filter_inside = false;
    // Additive (include/leann_backend.h "refining results on exact rows"): the walk fetches refine_fetch_k candidates (at least what
    // the search asks of the backend), they are scored again on the exact f32 rows of "<stem>.embeddings" and the best are kept: an int8
    // or bf16 index then returns the distances — hence the scores — an f32 index reports.  0 = off.  refine_rows_host: the exact rows
    // stay in pinned host memory that the kernel reads in place (the index keeps its share of the device memory); false: in HBM.
    // Hybrid mode is left alone: refine together with hybrid is refused.  `leann search --refine <FETCH_K> [--refine-rows hbm|host]`.
    size_t refine_fetch_k = 0;
    bool refine_rows_host = true;
    SearchOptions(size_t k, size_t c) : top_k(k), complexity(c) {}
    SearchOptions &with_refine(size_t fetch_k, bool rows_on_host = true) { refine_fetch_k = fetch_k; refine_rows_host = rows_on_host; return *this; }
    SearchOptions &with_device_filter(std::string key) { device_filter = true; filter_key = std::move(key); return *this; }
    SearchOptions &with_filter(MetadataFilter f) { filter = std::move(f); return *this; }
    SearchOptions &with_hybrid(std::string q, float alpha) { hybrid = true; hybrid_alpha = alpha; query_text = std::move(q); return *this; }
    SearchOptions &with_compat_polarity(bool on) { compat_polarity = on; return *this; }
    SearchOptions &with_bm25_device(bool on) { bm25_device = on; return *this; }
    SearchOptions &with_hybrid_filter_inside(bool on) { hybrid_filter_inside = on; return *this; }
};

inline std::vector<std::string> read_id_map(const std::string &index_path, const PassageStore &passages) {
    std::string ids_path = with_extension(index_path, "ids.txt"); // searcher.rs:83-92
    std::vector<std::string> ids;
    if (file_exists(ids_path)) {
        std::istringstream ss(read_file(ids_path));
        for (std::string line; std::getline(ss, line);) {
            if (!line.empty() && line.back() == '\r') line.pop_back();
            ids.push_back(line);
        }
    } else {
        ids = passages.ids();
    }
    return ids;
}

// leann_backend_append: a new backend handle over h's positions plus the n rows of `rows` ([n x dims], keys continue the sequence);
// `h` is left as it is.  Extending ids.txt, the passages and the meta file is the caller's (`leann update` is not part of this CLI).
inline std::shared_ptr<leann_backend> append_rows(const leann_backend *h, const std::vector<float> &rows, size_t n) {
    if (h && rows.size() != n * leann_backend_dims(h)) throw Error("append_rows: rows must hold n x dims floats");
    leann_backend *out = nullptr;
    check(leann_backend_append(h, n ? rows.data() : nullptr, n, &out));
    return std::shared_ptr<leann_backend>(out, leann_backend_close);
}

class IndexSearcher {
  public:
    static IndexSearcher load(const std::string &index_path, const IndexMeta &meta, const char *device = "0") {
        IndexSearcher s;
        s.passages_ = PassageStore::open(index_path);
        s.id_map_ = read_id_map(index_path, s.passages_);
        int backend;
        if (meta.backend_name == "hnsw") backend = LEANN_BACKEND_HNSW;
        else if (meta.backend_name == "diskann") backend = LEANN_BACKEND_DISKANN;
        else throw Error("Unknown backend: " + meta.backend_name); // searcher.rs:98
        leann_backend *h = nullptr;
        check(leann_backend_open(index_path.c_str(), backend, meta.dimensions, device, &h));
        s.backend_.reset(h, leann_backend_close);
        s.index_path_ = index_path;
        s.bm25_device_id_ = (int)std::strtol(device ? device : "0", nullptr, 10); // a list / range: its first device holds the result lists
        // removed positions (leann_backend_remove / `leann delete`), read once per handle: the backend never returns them, but BM25
        // is scored over every passage of the store and would bring them back through the hybrid branch
        if (leann_backend_live_len(h) != leann_backend_len(h)) {
            s.removed_.assign((leann_backend_len(h) + 7) / 8, 0);
            check(leann_backend_removed_bitmap(h, s.removed_.data(), nullptr));
        }
        return s;
    }
    // passages + id map only, no backend: assemble_results on recorded backend output (CPU tests)
    static IndexSearcher load_passages_only(const std::string &index_path) {
        IndexSearcher s;
        s.passages_ = PassageStore::open(index_path);
        s.id_map_ = read_id_map(index_path, s.passages_);
        return s;
    }
    std::vector<SearchResult> search(const std::vector<float> &q, size_t top_k, size_t complexity) const {
        return search_with_options(q, SearchOptions(top_k, complexity));
    }
    // searcher.rs:123-210
    std::vector<SearchResult> search_with_options(const std::vector<float> &query_embedding, const SearchOptions &opts) const {
        size_t fetch_k = (opts.filter || opts.hybrid) ? opts.top_k * 5 : opts.top_k; // :129-133
        std::vector<uint64_t> keys(std::max<size_t>(fetch_k, 1));
        std::vector<float> dists(std::max<size_t>(fetch_k, 1));
        size_t n = 0;
        if (query_embedding.size() != leann_backend_dims(backend_.get()))
            throw Error("query embedding has " + std::to_string(query_embedding.size()) + " dimensions, index has " +
                        std::to_string(leann_backend_dims(backend_.get())));
        if (opts.refine_fetch_k) { // the walk's candidates scored again on the exact rows; the score is the refined distance (N1, as below)
            auto lists = refined_lists(query_embedding.data(), 1, opts, fetch_k);
            return assemble_results(std::move(lists[0]), opts, fetch_k);
        }
        if (opts.filter && opts.device_filter) {
            // every returned position already passes the filter, so no over-fetch is needed for it
            if (!opts.hybrid) { fetch_k = opts.top_k; }
            // The filter lives on the device (bitmap + compacted list of allowed positions), registered once per distinct filter.
            const RegisteredFilter rf = device_filter(*opts.filter, opts.filter_key);
            const size_t complexity = filter_complexity(rf, opts.complexity, fetch_k);
            // mode 2: the library answers selective filters (<= 5 % of the rows, or <= 64k rows) exactly — the allowed rows are scanned
            // on the device — and walks otherwise.  One query at a time, 10M x 768 rows (scripts/filter_latency.py): 3 % allowed: 0.49 ms
            // exact against 0.80 ms walking at recall 0.92; 1 %: 0.32 ms against 1.8 ms at 0.84; 10 %: 1.1 ms against 0.46 ms at 0.89.
            uint32_t cnt = 0;
            check(leann_backend_search_filter_batch(backend_.get(), query_embedding.data(), 1, fetch_k, complexity, rf.handle.get(), 2,
                                                    keys.data(), dists.data(), &cnt));
            n = cnt;
        } else {
            check(leann_backend_search(backend_.get(), query_embedding.data(), fetch_k, opts.complexity, keys.data(), dists.data(), &n));
        }
        std::vector<std::pair<size_t, float>> vector_results;
        for (size_t i = 0; i < n; i++) vector_results.emplace_back((size_t)keys[i], dists[i]); // score = backend distance (N1)
        return assemble_results(std::move(vector_results), opts, fetch_k);
    }
    // Everything of search_with_options after the backend call (:146-207): hybrid merge, id map, passage fetch, post-filter, top_k cut.
    // Public so that the CPU suite can drive it with recorded backend output (tests/golden/searcher_cases.json, host_selftest).
    std::vector<SearchResult> assemble_results(std::vector<std::pair<size_t, float>> vector_results, const SearchOptions &opts,
                                               size_t fetch_k) const {
        if (opts.hybrid && opts.query_text) { // :146-169
            // The reference re-reads every passage and rebuilds the BM25 tables per query (:149-151, :213-224);
            // the index is immutable while open, so the tables are built once and kept —
            // scores are identical.
            const Bm25Scorer &scorer = bm25();
            leann_bm25 *dev = device_bm25_applies(opts, fetch_k) ? bm25_device(scorer) : nullptr;
            if (host_log_debug()) fprintf(stderr, "DEBUG leann: BM25 scored on the %s\n", dev ? "device" : "host");
            const std::shared_ptr<const HybridMask> mask = hybrid_mask(opts, scorer);
            if (host_log_debug() && mask) fprintf(stderr, "DEBUG leann: hybrid rerank under the allow-bitmap (%zu allowed)\n", mask->allowed);
            if (dev) {
                vector_results = device_hybrid(dev, scorer, {*opts.query_text}, {vector_results}, fetch_k, opts, mask ? mask->d_allow : nullptr)[0];
            } else if (mask) { // the definition of the leann_bm25_*_filtered calls on the host: same bits
                if (!opts.compat_polarity)
                    for (auto &r : vector_results) r.second = 1.0f - r.second;
                if (mask->allowed == 0) {
                    vector_results.clear(); // nothing is allowed: nothing comes back, whatever the ANN list holds
                } else {
                    auto bm25_scores = scorer.score_query(*opts.query_text);
                    std::vector<std::pair<size_t, float>> bm25_top;
                    for (size_t i = 0; i < bm25_scores.size(); i++)
                        if (bm25_scores[i] > 0.0f && mask->allows(i)) bm25_top.emplace_back(i, bm25_scores[i]);
                    std::stable_sort(bm25_top.begin(), bm25_top.end(), [](auto &a, auto &b) { return b.second < a.second; });
                    if (bm25_top.size() > fetch_k) bm25_top.resize(fetch_k);
                    std::unordered_set<size_t> have;
                    for (auto &r : vector_results) have.insert(r.first);
                    for (auto &b : bm25_top)
                        if (!have.count(b.first)) vector_results.emplace_back(b.first, 0.0f);
                    vector_results = hybrid_rerank(vector_results, bm25_scores, opts.hybrid_alpha, &mask->host);
                }
            } else {
                if (!opts.compat_polarity)
                    for (auto &r : vector_results) r.second = 1.0f - r.second; // corrected polarity (N1): similarity, larger = better
                auto bm25_scores = scorer.score_query(*opts.query_text);
                auto bm25_top = scorer.search(*opts.query_text, fetch_k);
                std::unordered_set<size_t> have;
                for (auto &r : vector_results) have.insert(r.first);
                for (auto &b : bm25_top)
                    if (!have.count(b.first) && !is_removed(b.first)) vector_results.emplace_back(b.first, 0.0f); // (no BM25-only hit at a removed position)
                vector_results = hybrid_rerank(vector_results, bm25_scores, opts.hybrid_alpha);
            }
        }
        return finish_results(vector_results, opts);
    }
    // search_with_options for many queries (hybrid mode, no metadata filter inside the traversal): one batched backend search and ONE
    // leann_bm25_hybrid_rerank_device call for the whole batch; per query the result of search_with_options.
    std::vector<std::vector<SearchResult>> search_batch_with_options(const std::vector<std::vector<float>> &query_embeddings,
                                                                     const std::vector<std::string> &query_texts,
                                                                     const SearchOptions &opts) const {
        const size_t nq = query_embeddings.size(), dims = leann_backend_dims(backend_.get());
        if (query_texts.size() != nq) throw Error("search_batch_with_options: one query text per embedding is required");
        if (opts.refine_fetch_k) { // one walk and one rerank for the whole batch; per query the result of search_with_options
            std::vector<float> q(nq * dims);
            for (size_t i = 0; i < nq; i++) {
                if (query_embeddings[i].size() != dims)
                    throw Error("query embedding has " + std::to_string(query_embeddings[i].size()) + " dimensions, index has " + std::to_string(dims));
                std::copy(query_embeddings[i].begin(), query_embeddings[i].end(), q.begin() + i * dims);
            }
            std::vector<std::vector<SearchResult>> refined;
            for (auto &list : refined_lists(q.data(), nq, opts, opts.filter ? opts.top_k * 5 : opts.top_k)) refined.push_back(finish_results(list, opts));
            return refined;
        }
        const size_t fetch_k = opts.top_k * 5;
        leann_bm25 *dev = (opts.hybrid && device_bm25_applies(opts, fetch_k)) ? bm25_device(bm25()) : nullptr;
        std::vector<std::vector<SearchResult>> out;
        const bool filter_inside = opts.hybrid && opts.hybrid_filter_inside && opts.filter && opts.device_filter && dev;
        if (!opts.hybrid || (opts.filter && opts.device_filter && !filter_inside) || !dev) { // nothing to batch: the single-query path, query by query
            for (size_t i = 0; i < nq; i++) {
                SearchOptions o = opts;
                if (opts.hybrid) o.query_text = query_texts[i];
                out.push_back(search_with_options(query_embeddings[i], o));
            }
            return out;
        }
        std::vector<float> q(nq * dims);
        for (size_t i = 0; i < nq; i++) {
            if (query_embeddings[i].size() != dims)
                throw Error("query embedding has " + std::to_string(query_embeddings[i].size()) + " dimensions, index has " + std::to_string(dims));
            std::copy(query_embeddings[i].begin(), query_embeddings[i].end(), q.begin() + i * dims);
        }
        std::vector<uint64_t> keys(nq * fetch_k);
        std::vector<float> dists(nq * fetch_k);
        std::vector<uint32_t> counts(nq);
        std::shared_ptr<const HybridMask> mask = hybrid_mask(opts, bm25());
        if (filter_inside) {
            // the filtered search of search_with_options for the whole batch.  The library chooses between the walk and the exact scan
            // by the batch size too (64 queries is the line), so the batch goes in groups of at most 64: every query is answered as
            // it is alone.  One rerank call for all of them follows.
            const RegisteredFilter rf = device_filter(*opts.filter, opts.filter_key);
            const size_t complexity = filter_complexity(rf, opts.complexity, fetch_k);
            for (size_t q0 = 0; q0 < nq; q0 += 64) {
                const size_t m = std::min<size_t>(64, nq - q0);
                check(leann_backend_search_filter_batch(backend_.get(), q.data() + q0 * dims, m, fetch_k, complexity, rf.handle.get(), 2,
                                                        keys.data() + q0 * fetch_k, dists.data() + q0 * fetch_k, counts.data() + q0));
            }
        } else {
            check(leann_backend_search_batch(backend_.get(), q.data(), nq, fetch_k, opts.complexity, keys.data(), dists.data(), counts.data()));
        }
        std::vector<std::vector<std::pair<size_t, float>>> lists(nq);
        for (size_t i = 0; i < nq; i++)
            for (size_t j = 0; j < counts[i]; j++) lists[i].emplace_back((size_t)keys[i * fetch_k + j], dists[i * fetch_k + j]);
        if (host_log_debug()) fprintf(stderr, "DEBUG leann: BM25 scored on the device (batch of %zu)\n", nq);
        if (host_log_debug() && mask) fprintf(stderr, "DEBUG leann: hybrid rerank under the allow-bitmap (%zu allowed)\n", mask->allowed);
        auto reranked = device_hybrid(dev, bm25(), query_texts, lists, fetch_k, opts, mask ? mask->d_allow : nullptr);
        for (size_t i = 0; i < nq; i++) out.push_back(finish_results(reranked[i], opts));
        return out;
    }
    // :171-207 — id map, passage fetch, post-filter, top_k cut
    std::vector<SearchResult> finish_results(const std::vector<std::pair<size_t, float>> &vector_results, const SearchOptions &opts) const {
        std::vector<SearchResult> results;
        for (auto &r : vector_results) {
            if (results.size() >= opts.top_k) break;
            if (is_removed(r.first)) continue; // (the device BM25 path injects inside the kernel: masked here, like the host path's injection)
            std::string id = r.first < id_map_.size() ? id_map_[r.first] : std::to_string(r.first); // :180-184
            try {
                Passage p = passages_.get(id);
                if (opts.filter && !opts.filter->matches(p.metadata)) continue;
                results.push_back({id, r.second, p.text, p.metadata});
            } catch (const std::exception &e) {
                fprintf(stderr, "WARN Failed to load passage %s: %s\n", id.c_str(), e.what());
            }
        }
        return results;
    }
    std::vector<std::string> get_all_texts() const { // :213-224
        std::vector<std::string> texts;
        texts.reserve(id_map_.size());
        for (auto &id : id_map_) {
            try { texts.push_back(passages_.get(id).text); } catch (...) { texts.emplace_back(); }
        }
        return texts;
    }
    std::vector<std::string> bm25_search(const std::string &query, size_t top_k) const { // :228-246
        const Bm25Scorer &scorer = bm25();
        std::vector<std::string> texts;
        for (auto &r : scorer.search(query, top_k))
            if (r.first < id_map_.size()) {
                try { texts.push_back(passages_.get(id_map_[r.first]).text); } catch (...) {}
            }
        return texts;
    }
    size_t len() const { return leann_backend_len(backend_.get()); }
    bool is_empty() const { return len() == 0; }

  private:
    // `want` results per query from the walk at max(refine_fetch_k, want) candidates, refined on the exact rows (opened on first use)
    std::vector<std::vector<std::pair<size_t, float>>> refined_lists(const float *q, size_t nq, const SearchOptions &opts, size_t want) const {
        if (opts.hybrid)
            throw Error("--refine together with --hybrid is not supported: the hybrid rerank blends the walk's distances, and refining "
                        "inside it is a follow-up; drop one of the two");
        if (opts.filter && opts.device_filter)
            throw Error("--refine together with --device-filter is not supported yet; without --device-filter the filter acts after the refined search");
        want = std::max<size_t>(want, 1);
        const size_t fetch_k = std::max(opts.refine_fetch_k, want);
        std::vector<uint64_t> keys(nq * want);
        std::vector<float> dists(nq * want);
        std::vector<uint32_t> counts(nq);
        check(leann_backend_search_refined_batch(backend_.get(), exact_rows(opts.refine_rows_host), q, nq, want, fetch_k, opts.complexity, nullptr,
                                                 0, keys.data(), dists.data(), counts.data(), nullptr));
        std::vector<std::vector<std::pair<size_t, float>>> lists(nq);
        for (size_t i = 0; i < nq; i++)
            for (size_t j = 0; j < counts[i]; j++) lists[i].emplace_back((size_t)keys[i * want + j], dists[i * want + j]);
        return lists;
    }
    const leann_exact_rows *exact_rows(bool on_host) const {
        std::lock_guard<std::mutex> lk(*bm25_mu_);
        std::shared_ptr<leann_exact_rows> &slot = exact_->handle[on_host ? 1 : 0];
        if (!slot) {
            const std::string emb = with_extension(index_path_, "embeddings");
            if (!file_exists(emb))
                throw Error("--refine needs the exact rows, and " + emb + " does not exist: build the index with `leann build --recompute`, "
                            "which writes them beside the index");
            leann_exact_rows *raw = nullptr;
            check(leann_exact_rows_open(emb.c_str(), leann_backend_dims(backend_.get()), bm25_device_id_, 0,
                                        on_host ? LEANN_EXACT_ROWS_HOST : LEANN_EXACT_ROWS_HBM, &raw));
            slot.reset(raw, leann_exact_rows_close);
            if (host_log_debug())
                fprintf(stderr, "DEBUG leann: %zu exact rows of %s kept in %s\n", leann_exact_rows_len(raw), emb.c_str(), on_host ? "pinned host memory" : "HBM");
        }
        return slot.get();
    }
    bool is_removed(size_t pos) const { return (pos >> 3) < removed_.size() && ((removed_[pos >> 3] >> (pos & 7)) & 1); }
    const Bm25Scorer &bm25() const {
        std::lock_guard<std::mutex> lk(*bm25_mu_);
        if (!bm25_) bm25_ = std::make_shared<Bm25Scorer>(Bm25Scorer::build(get_all_texts()));
        return *bm25_;
    }
    static bool host_log_debug() {
        const char *e = getenv("LEANN_LOG");
        return e && !strcmp(e, "debug");
    }
    // The device call takes what the reference's arithmetic is pinned for: fetch_k <= 256 and alpha in [0, 1].  The reference itself
    // accepts any f32 alpha (searcher.rs:57-59, bm25.rs:163), NaN included: such a query is scored on the host, as before.
    bool device_bm25_applies(const SearchOptions &opts, size_t fetch_k) const {
        return opts.bm25_device && backend_ && fetch_k >= 1 && fetch_k <= 256 && opts.hybrid_alpha >= 0.0f && opts.hybrid_alpha <= 1.0f;
    }
    // the scorer's inverted index on the device, created on first use and shared by every copy of this searcher; null when there is no
    // device, no passage, or the handle could not be created (logged once): BM25 is then scored on the host, same bits
    leann_bm25 *bm25_device(const Bm25Scorer &scorer) const {
        std::lock_guard<std::mutex> lk(*bm25_mu_);
        if (bm25_dev_->handle || bm25_dev_->tried) return bm25_dev_->handle.get();
        bm25_dev_->tried = true;
        int ndev = 0;
        if (scorer.num_docs() == 0 || leann_device_count(&ndev) != LEANN_OK || ndev < 1) return nullptr;
        std::vector<uint64_t> off;
        std::vector<uint32_t> doc, tf, len;
        scorer.export_csr(off, doc, tf, len);
        leann_bm25 *raw = nullptr;
        if (leann_bm25_create(scorer.num_docs(), scorer.num_terms(), off.data(), doc.data(), tf.data(), len.data(), scorer.avg_doc_len(),
                              bm25_device_id_, &raw) != LEANN_OK) {
            fprintf(stderr, "WARN BM25 index not created on the device, scoring on the host: %s\n", leann_last_error());
            return nullptr;
        }
        bm25_dev_->handle.reset(raw, leann_bm25_close);
        return raw;
    }
    struct DeviceBuf { // HBM block on the BM25 handle's device, freed on scope exit
        void *p = nullptr;
        DeviceBuf(int device, size_t bytes) { check(leann_device_malloc(device, std::max<size_t>(bytes, 16), &p)); }
        ~DeviceBuf() { if (p) leann_device_free(p); }
        DeviceBuf(const DeviceBuf &) = delete;
        DeviceBuf &operator=(const DeviceBuf &) = delete;
    };
    // searcher.rs:146-169 for a batch on the device: backend lists (key, DISTANCE) up, merged + reranked lists (all of them) down
    std::vector<std::vector<std::pair<size_t, float>>> device_hybrid(leann_bm25 *dev, const Bm25Scorer &scorer,
                                                                     const std::vector<std::string> &texts,
                                                                     const std::vector<std::vector<std::pair<size_t, float>>> &lists,
                                                                     size_t fetch_k, const SearchOptions &opts,
                                                                     const uint8_t *d_allow = nullptr) const {
        const size_t nq = lists.size(), out_k = 2 * fetch_k; // the merged list has at most fetch_k + fetch_k entries
        std::vector<uint32_t> q_off(1, 0), q_term, counts(nq);
        std::vector<float> q_idf;
        std::vector<uint64_t> keys(nq * fetch_k, ~0ull);
        std::vector<float> dists(nq * fetch_k, INFINITY);
        for (size_t i = 0; i < nq; i++) {
            for (auto &t : scorer.query_terms(texts[i])) { q_term.push_back(t.first); q_idf.push_back(t.second); }
            q_off.push_back((uint32_t)q_term.size());
            counts[i] = (uint32_t)std::min(lists[i].size(), fetch_k);
            for (size_t j = 0; j < counts[i]; j++) { keys[i * fetch_k + j] = lists[i][j].first; dists[i * fetch_k + j] = lists[i][j].second; }
        }
        const int d = bm25_device_id_;
        DeviceBuf dk(d, keys.size() * 8), dd(d, dists.size() * 4), dc(d, nq * 4), ok(d, nq * out_k * 8), os(d, nq * out_k * 4), oc(d, nq * 4);
        check(leann_device_upload(dk.p, keys.data(), keys.size() * 8));
        check(leann_device_upload(dd.p, dists.data(), dists.size() * 4));
        check(leann_device_upload(dc.p, counts.data(), nq * 4));
        if (d_allow)
            check(leann_bm25_hybrid_rerank_filtered_device(dev, nq, q_off.data(), q_term.data(), q_idf.data(), (const uint64_t *)dk.p,
                                                           (const float *)dd.p, (const uint32_t *)dc.p, fetch_k, opts.hybrid_alpha,
                                                           opts.compat_polarity ? 1 : 0, out_k, d_allow, 0, (uint64_t *)ok.p, (float *)os.p,
                                                           (uint32_t *)oc.p, nullptr));
        else
            check(leann_bm25_hybrid_rerank_device(dev, nq, q_off.data(), q_term.data(), q_idf.data(), (const uint64_t *)dk.p, (const float *)dd.p,
                                                  (const uint32_t *)dc.p, fetch_k, opts.hybrid_alpha, opts.compat_polarity ? 1 : 0, out_k,
                                                  (uint64_t *)ok.p, (float *)os.p, (uint32_t *)oc.p, nullptr));
        std::vector<uint64_t> rk(nq * out_k);
        std::vector<float> rs(nq * out_k);
        std::vector<uint32_t> rc(nq);
        check(leann_device_download(rk.data(), ok.p, rk.size() * 8));
        check(leann_device_download(rs.data(), os.p, rs.size() * 4));
        check(leann_device_download(rc.data(), oc.p, nq * 4));
        std::vector<std::vector<std::pair<size_t, float>>> out(nq);
        for (size_t i = 0; i < nq; i++)
            for (size_t j = 0; j < rc[i]; j++) out[i].emplace_back((size_t)rk[i * out_k + j], rs[i * out_k + j]);
        return out;
    }
    // one pass over the passage metadata per distinct filter (the index is immutable while open); bit i = position i.  The bitmap is
    // registered on the device once (leann_backend_filter_create) and reused by every query under the same filter.
    struct RegisteredFilter {
        std::shared_ptr<leann_filter> handle;
        size_t allowed = 0;
    };
    RegisteredFilter device_filter(const MetadataFilter &f, const std::string &key) const { // by value: keeps the handle alive past an eviction
        std::lock_guard<std::mutex> lk(*bm25_mu_);
        if (!key.empty()) {
            auto it = filters_->find(key);
            if (it != filters_->end()) return it->second;
        }
        const size_t n = leann_backend_len(backend_.get());
        leann_filter *raw = nullptr;
        const auto t0 = std::chrono::steady_clock::now();
        auto ms = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
        if (!leann_meta_device_enabled()) {
            if (host_log_debug()) fprintf(stderr, "DEBUG leann: filter evaluated on the host, passage by passage (LEANN_META_DEVICE=0)\n");
        } else if (meta_filter(f, n, &raw)) {
            if (host_log_debug())
                fprintf(stderr, "DEBUG leann: filter evaluated on the device from %zu metadata columns, registered in %.3f ms\n", meta_->fields.size(), ms());
            return remember(key, raw);
        } else if (host_log_debug()) fprintf(stderr, "DEBUG leann: filter evaluated on the host, passage by passage: %s\n", leann_last_error());
        std::vector<uint8_t> bm((n + 7) / 8 + 1, 0);
        for (size_t i = 0; i < n; i++) {
            std::string id = i < id_map_.size() ? id_map_[i] : std::to_string(i);
            try {
                if (f.matches(passages_.get(id).metadata)) bm[i >> 3] |= (uint8_t)(1u << (i & 7));
            } catch (...) {} // unreadable passage: never returned (the post-filter path skips it with a warning too)
        }
        check(leann_backend_filter_create(backend_.get(), bm.data(), &raw));
        if (host_log_debug()) fprintf(stderr, "DEBUG leann: host pass over %zu passages, filter registered in %.3f ms\n", n, ms());
        return remember(key, raw);
    }
    // The walk answers from the pool of evaluated nodes (20-33 x complexity for M = 16-32): widen it so that the pool is
    // expected to hold >= 8 x fetch_k allowed passages (selectivity s: complexity >= 8 fetch_k / (20 s)), capped at 1024.
    size_t filter_complexity(const RegisteredFilter &rf, size_t complexity, size_t fetch_k) const {
        const size_t n_rows = std::max<size_t>(leann_backend_len(backend_.get()), 1);
        if (rf.allowed > 0) {
            const double s_sel = (double)rf.allowed / (double)n_rows;
            complexity = std::min<size_t>(1024, std::max<size_t>(complexity, (size_t)std::ceil(8.0 * (double)fetch_k / (20.0 * s_sel))));
        }
        return complexity;
    }
    RegisteredFilter remember(const std::string &key, leann_filter *raw) const {
        RegisteredFilter rf;
        rf.handle = std::shared_ptr<leann_filter>(raw, [](leann_filter *p) { leann_backend_filter_free(p); });
        rf.allowed = leann_backend_filter_count(raw);
        if (filters_->size() >= 16) filters_->clear();
        return (*filters_)[key.empty() ? std::string("\x01anon") : key] = std::move(rf);
    }
    // `--hybrid-filter inside`: what the BM25 half of a hybrid query may see — the registered filter's bitmap (valid AND match AND live)
    // under --device-filter, else the live positions of an index with removals (an all-ones filter, registered once: the handle's
    // removals do not change while the index is open); null when neither applies or the mode is off.  d_allow is on the BM25 handle's
    // device: the registered bitmap itself (leann_backend_filter_bitmap_device), or, for a composite handle, whose filter has no whole
    // bitmap, a copy made here from the per-passage loop and kept with the entry.  `host` is the same bitmap for the host BM25 path.
    struct HybridMask {
        RegisteredFilter filter;      // keeps the registered bitmap alive
        std::shared_ptr<void> own;    // a composite handle: the copy on the first device
        const uint8_t *d_allow = nullptr;
        std::vector<uint8_t> host;
        size_t allowed = 0;
        bool allows(size_t i) const { return (i >> 3) < host.size() && ((host[i >> 3] >> (i & 7)) & 1); }
    };
    std::shared_ptr<const HybridMask> hybrid_mask(const SearchOptions &opts, const Bm25Scorer &scorer) const {
        if (!opts.hybrid || !opts.hybrid_filter_inside || !backend_) return nullptr;
        const bool by_filter = opts.filter && opts.device_filter;
        if (!by_filter && removed_.empty()) return nullptr;
        const size_t n = leann_backend_len(backend_.get());
        if (scorer.num_docs() != n) { // the bitmap is over the backend's positions
            fprintf(stderr, "WARN --hybrid-filter inside: %zu passages, %zu index rows; the filter acts after the rerank\n", scorer.num_docs(), n);
            return nullptr;
        }
        const std::string key = by_filter ? (opts.filter_key.empty() ? std::string("\x01anon") : opts.filter_key) : std::string("\x02live");
        {
            std::lock_guard<std::mutex> lk(*bm25_mu_);
            auto it = masks_->find(key);
            if (it != masks_->end() && (!by_filter || !opts.filter_key.empty())) return it->second;
        }
        auto m = std::make_shared<HybridMask>();
        const size_t nbytes = (n + 7) / 8;
        if (by_filter) {
            m->filter = device_filter(*opts.filter, opts.filter_key);
        } else {
            std::vector<uint8_t> ones(nbytes + 1, 0xFF);
            leann_filter *raw = nullptr;
            check(leann_backend_filter_create(backend_.get(), ones.data(), &raw)); // ANDs the live mask
            m->filter.handle = std::shared_ptr<leann_filter>(raw, [](leann_filter *p) { leann_backend_filter_free(p); });
            m->filter.allowed = leann_backend_filter_count(raw);
        }
        m->allowed = m->filter.allowed;
        m->host.assign(nbytes, 0);
        size_t n_pos = 0;
        const int rc = leann_backend_filter_bitmap_device(m->filter.handle.get(), &m->d_allow, &n_pos);
        if (rc == LEANN_OK) {
            if (n_pos != n) throw Error("registered filter covers " + std::to_string(n_pos) + " positions, the index has " + std::to_string(n));
            check(leann_device_download(m->host.data(), const_cast<uint8_t *>(m->d_allow), nbytes));
        } else if (rc == LEANN_ERR_UNSUPPORTED) { // a composite handle: the bitmap over global positions, made here, on the first device
            for (size_t i = 0; i < n; i++) {
                if (is_removed(i)) continue;
                bool ok = !by_filter;
                if (by_filter) {
                    std::string id = i < id_map_.size() ? id_map_[i] : std::to_string(i);
                    try { ok = opts.filter->matches(passages_.get(id).metadata); } catch (...) {}
                }
                if (ok) m->host[i >> 3] |= (uint8_t)(1u << (i & 7));
            }
            void *p = nullptr;
            check(leann_device_malloc(bm25_device_id_, std::max<size_t>(nbytes, 16), &p));
            m->own = std::shared_ptr<void>(p, [](void *q) { leann_device_free(q); });
            check(leann_device_upload(p, m->host.data(), nbytes));
            m->d_allow = (const uint8_t *)p;
        } else {
            check(rc);
        }
        std::lock_guard<std::mutex> lk(*bm25_mu_);
        if (masks_->size() >= 16) masks_->clear();
        (*masks_)[key] = m;
        return m;
    }
    // The device path of device_filter (include/leann_backend.h "metadata filters evaluated on the device"): the open index keeps one
    // columnar store; a field gets its column the first time a filter names it, by ONE pass over the passages that extracts the fields
    // still missing (the store's own first pass also records which passages could be read); after that a new filter costs a compile
    // and a kernel, no passage is touched.  false (leann_last_error says why): the store could not be made or the filter exceeds a
    // limit of the compiler — the caller falls back to the per-passage loop.  Called under bm25_mu_.
    struct MetaStore {
        std::shared_ptr<leann_meta> handle;
        bool failed = false;
        std::vector<std::string> fields;
    };
    static const lj::Value *nested(const lj::Value &metadata, const std::string &path) { // get_nested_value, filter.rs:376-388
        const lj::Value *v = &metadata;
        size_t start = 0;
        for (;;) {
            const size_t dot = path.find('.', start);
            v = v->get(path.substr(start, dot == std::string::npos ? std::string::npos : dot - start));
            if (!v || dot == std::string::npos) return v;
            start = dot + 1;
        }
    }
    static void collect_fields(const MetadataFilter &f, std::vector<std::string> &out) {
        if (!f.is_condition()) { for (auto &c : f.children()) collect_fields(c, out); return; }
        if (std::find(out.begin(), out.end(), f.field()) == out.end()) out.push_back(f.field());
    }
    static leann_meta_value meta_value(const lj::Value &v, std::deque<std::vector<leann_meta_value>> &lists, bool in_list = false) {
        leann_meta_value out{};
        switch (v.kind) {
        case lj::Value::Null: out.type = LEANN_META_VAL_NULL; break;
        case lj::Value::Bool: out.type = LEANN_META_VAL_BOOL; out.boolean = v.b; break;
        case lj::Value::Int:
        case lj::Value::Float: out.type = LEANN_META_VAL_NUMBER; out.num = v.as_f64(); break;
        case lj::Value::String: out.type = LEANN_META_VAL_STRING; out.str = v.s.data(); out.len = v.s.size(); break;
        default: // an array; an element that is itself an array (or an object) equals nothing: an empty list
            out.type = LEANN_META_VAL_LIST;
            if (!in_list && v.kind == lj::Value::Arr) {
                lists.emplace_back();
                std::vector<leann_meta_value> &l = lists.back();
                for (auto &x : *v.a) l.push_back(meta_value(x, lists, true));
                out.len = l.size();
                out.list = l.data();
            }
        }
        return out;
    }
    static void flatten(const MetadataFilter &f, std::vector<leann_meta_node> &nodes, std::deque<std::vector<leann_meta_value>> &lists) {
        leann_meta_node nd{};
        if (f.is_condition()) {
            nd.kind = LEANN_META_COND;
            nd.field = f.field().c_str();
            nd.op = (int32_t)f.op(); // MetadataFilter::Op is in the order of LEANN_META_OP_*
            nd.value = meta_value(f.value(), lists);
            nodes.push_back(nd);
            return;
        }
        nd.kind = f.is_and() ? LEANN_META_AND : LEANN_META_OR;
        nd.n_children = (uint32_t)f.children().size();
        nodes.push_back(nd);
        for (auto &c : f.children()) flatten(c, nodes, lists);
    }
    bool meta_filter(const MetadataFilter &f, size_t n, leann_filter **out) const {
        if (meta_->failed) return false;
        std::vector<std::string> fields, missing;
        collect_fields(f, fields);
        for (auto &fl : fields)
            if (std::find(meta_->fields.begin(), meta_->fields.end(), fl) == meta_->fields.end()) missing.push_back(fl);
        const bool first = !meta_->handle;
        if (first || !missing.empty()) { // one pass over the passages: the missing fields' columns, and readability the first time
            std::vector<uint8_t> valid((n + 7) / 8 + 1, 0);
            std::vector<std::vector<uint8_t>> tag(missing.size(), std::vector<uint8_t>(n, LEANN_META_MISSING));
            std::vector<std::vector<double>> num(missing.size(), std::vector<double>(n, 0.0));
            std::vector<std::string> blob(missing.size());
            std::vector<std::vector<uint64_t>> off(missing.size(), std::vector<uint64_t>(n + 1, 0));
            for (size_t i = 0; i < n; i++) {
                const std::string id = i < id_map_.size() ? id_map_[i] : std::to_string(i);
                try {
                    const lj::Value metadata = passages_.get(id).metadata;
                    valid[i >> 3] |= (uint8_t)(1u << (i & 7));
                    for (size_t c = 0; c < missing.size(); c++) {
                        const lj::Value *v = nested(metadata, missing[c]);
                        uint8_t t = LEANN_META_OTHER;
                        if (!v) t = LEANN_META_MISSING;
                        else if (v->is_null()) t = LEANN_META_NULL;
                        else if (v->kind == lj::Value::Bool) t = v->b ? LEANN_META_TRUE : LEANN_META_FALSE;
                        else if (v->is_number()) { t = LEANN_META_NUMBER; num[c][i] = v->as_f64(); }
                        else if (v->is_string()) { t = LEANN_META_STRING; blob[c] += v->s; }
                        tag[c][i] = t;
                    }
                } catch (...) {} // unreadable passage: invalid, passes no filter
                for (size_t c = 0; c < missing.size(); c++) off[c][i + 1] = blob[c].size();
            }
            if (first) {
                leann_meta *m = nullptr;
                if (leann_meta_create(n, valid.data(), bm25_device_id_, &m) != LEANN_OK) { meta_->failed = true; return false; }
                meta_->handle.reset(m, leann_meta_close);
            }
            for (size_t c = 0; c < missing.size(); c++) {
                if (leann_meta_add_column(meta_->handle.get(), missing[c].c_str(), tag[c].data(), num[c].data(), blob[c].data(), off[c].data()) != LEANN_OK)
                    return false;
                meta_->fields.push_back(missing[c]);
            }
        }
        std::vector<leann_meta_node> nodes;
        std::deque<std::vector<leann_meta_value>> lists;
        flatten(f, nodes, lists);
        return leann_backend_filter_create_meta(backend_.get(), meta_->handle.get(), nodes.data(), nodes.size(), out) == LEANN_OK;
    }
    std::shared_ptr<MetaStore> meta_ = std::make_shared<MetaStore>();
    PassageStore passages_;
    std::shared_ptr<leann_backend> backend_;
    std::string index_path_;
    struct ExactRows { std::shared_ptr<leann_exact_rows> handle[2]; }; // [0] in HBM, [1] in pinned host memory; opened by the first refined search
    std::shared_ptr<ExactRows> exact_ = std::make_shared<ExactRows>();
    std::vector<std::string> id_map_;
    std::vector<uint8_t> removed_; // bitmap of removed positions; empty when nothing is removed
    std::shared_ptr<std::map<std::string, RegisteredFilter>> filters_ = std::make_shared<std::map<std::string, RegisteredFilter>>();
    std::shared_ptr<std::map<std::string, std::shared_ptr<const HybridMask>>> masks_ =
        std::make_shared<std::map<std::string, std::shared_ptr<const HybridMask>>>();
    mutable std::shared_ptr<Bm25Scorer> bm25_;
    struct Bm25Device { // the scorer's postings in HBM; one per loaded index, shared by its copies like the mutex that guards it
        std::shared_ptr<leann_bm25> handle;
        bool tried = false;
    };
    std::shared_ptr<Bm25Device> bm25_dev_ = std::make_shared<Bm25Device>();
    int bm25_device_id_ = 0;
    std::shared_ptr<std::mutex> bm25_mu_ = std::make_shared<std::mutex>();
};

// ---- embeddings: the thing RecomputeSearcher calls (src/embedding/mod.rs:112-143) ------------------------
// Every real provider of the reference needs the network (OpenAI / Ollama / Gemini HTTP, HF hub);
// offline the host offers a deterministic "synthetic" text embedder (hashed token directions,
// L2-normalised like every registry model, src/embedding/models.rs:39-120) and raw vector files.
inline uint64_t mix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
inline std::vector<float> synthetic_embed(const std::string &text, size_t dims) {
    std::vector<float> v(dims, 0.0f);
    auto toks = tokenize(text);
    if (toks.empty()) toks.push_back(text);
    for (auto &t : toks) {
        uint64_t h = 0xcbf29ce484222325ull;
        for (unsigned char c : t) h = (h ^ c) * 0x100000001b3ull;
        for (size_t j = 0; j < dims; j++) {
            uint64_t r = mix64(mix64(h) ^ (j * 0xA24BAED4963EE407ull));
            int32_t s = (int32_t)((r & 0xFFFF) + ((r >> 16) & 0xFFFF) + ((r >> 32) & 0xFFFF) + (r >> 48));
            v[j] += (float)(s - 131070) * 2.6428996e-05f;
        }
    }
    float ss = 0.0f;
    for (float x : v) ss += x * x;
    float nrm = std::sqrt(ss);
    if (nrm < 1e-12f) nrm = 1e-12f; // candle.rs:218-225
    for (float &x : v) x /= nrm;
    return v;
}
// "synthetic-linear": the recompute path's device-resident provider fed from text — compact per-passage features
// + a dense layer + L2 normalisation (the tail of a real encoder, candle.rs:165,218-225):
//     f = signed hashed bag of tokens [LINEAR_H]  (small integers: exact in bf16),   W [LINEAR_H x dims] bf16, seeded Gaussian,
//     embedding = l2_normalize(W^T f).
// An index built with `--recompute-graph` stores the graph and the features (520 B per passage), never the embeddings; the host
// only embeds the QUERY text (this function), distances are recomputed on the device during the walk.
constexpr size_t LINEAR_H = 256;
inline uint16_t bf16_rne(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
inline float bf16_to_f32(uint16_t b) {
    uint32_t u = (uint32_t)b << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
inline std::vector<uint16_t> linear_features(const std::string &text) {
    std::vector<float> f(LINEAR_H, 0.0f);
    auto toks = tokenize(text);
    if (toks.empty()) toks.push_back(text);
    for (auto &t : toks) {
        uint64_t h = 0xcbf29ce484222325ull;
        for (unsigned char c : t) h = (h ^ c) * 0x100000001b3ull;
        for (int rep = 0; rep < 4; rep++) { // four signed buckets per token: fewer collisions between distinct tokens
            const uint64_t r = mix64(h + (uint64_t)rep * 0x9E3779B97F4A7C15ull);
            f[r % LINEAR_H] += (r >> 63) ? 1.0f : -1.0f;
        }
    }
    std::vector<uint16_t> out(LINEAR_H);
    for (size_t k = 0; k < LINEAR_H; k++) out[k] = bf16_rne(f[k]);
    return out;
}
inline std::vector<uint16_t> linear_weights(size_t dims) { // [LINEAR_H x dims] bf16, row-major
    std::vector<uint16_t> W(LINEAR_H * dims);
    for (size_t k = 0; k < LINEAR_H; k++)
        for (size_t j = 0; j < dims; j++) {
            const uint64_t r = mix64(mix64(0x4C494E454152ull ^ (k * 0xD1342543DE82EF95ull)) ^ (j * 0xA24BAED4963EE407ull));
            const int32_t sgn = (int32_t)((r & 0xFFFF) + ((r >> 16) & 0xFFFF) + ((r >> 32) & 0xFFFF) + (r >> 48));
            W[k * dims + j] = bf16_rne((float)(sgn - 131070) * 2.6428996e-05f);
        }
    return W;
}
inline std::vector<float> linear_embed(const std::string &text, const std::vector<uint16_t> &W, size_t dims) {
    const auto f = linear_features(text);
    std::vector<float> e(dims, 0.0f);
    for (size_t k = 0; k < LINEAR_H; k++) {
        const float fk = bf16_to_f32(f[k]);
        if (fk == 0.0f) continue;
        for (size_t j = 0; j < dims; j++) e[j] = std::fma(bf16_to_f32(W[k * dims + j]), fk, e[j]);
    }
    float ss = 0.0f;
    for (float x : e) ss += x * x;
    float nrm = std::sqrt(ss);
    if (nrm < 1e-12f) nrm = 1e-12f;
    for (float &x : e) x /= nrm;
    return e;
}

class EmbeddingProvider {
  public:
    EmbeddingProvider(std::string mode, size_t dims) : mode_(std::move(mode)), dims_(dims) {
        if (mode_ != "synthetic" && mode_ != "synthetic-linear")
            throw Error("Embedding mode '" + mode_ + "' needs a network service that is unavailable in this build; "
                        "use --embedding-mode synthetic or --query-vector-file");
        if (mode_ == "synthetic-linear") weights_ = linear_weights(dims_);
    }
    std::vector<std::vector<float>> embed(const std::vector<std::string> &texts) const {
        std::vector<std::vector<float>> out;
        for (auto &t : texts) out.push_back(weights_.empty() ? synthetic_embed(t, dims_) : linear_embed(t, weights_, dims_));
        return out;
    }
    std::vector<std::vector<float>> embed_with_template(const std::vector<std::string> &texts, const std::string &tmpl) const {
        std::vector<std::string> t2;
        for (auto &t : texts) t2.push_back(tmpl + t); // embedding/mod.rs:126-143 prefix templating
        return embed(t2);
    }
    size_t dimensions() const { return dims_; }
    const std::vector<uint16_t> &weights() const { return weights_; } // synthetic-linear: W [LINEAR_H x dims] bf16

  private:
    std::string mode_;
    size_t dims_;
    std::vector<uint16_t> weights_;
};

// ---- src/index/recompute.rs ---------------------------------------------------------------------------
// Pruned index: brute force over re-embedded passages.  Texts are collected (with the early filter,
// :62-79) and embedded in batches of 100 (:86-93) on the host-side provider; the N dot products, the
// stable descending sort and take(k) (:96-109) run on the GPU (leann_scan_topk_device).
class RecomputeSearcher {
  public:
    static RecomputeSearcher load(const std::string &index_path, size_t dimensions) {
        RecomputeSearcher s;
        s.passages_ = PassageStore::open(index_path);
        s.id_map_ = read_id_map(index_path, s.passages_);
        s.dimensions_ = dimensions;
        return s;
    }
    std::vector<SearchResult> search(const std::vector<float> &query_embedding, const EmbeddingProvider &provider, size_t top_k,
                                     const MetadataFilter *filter) const {
        std::vector<std::string> texts;
        std::vector<size_t> valid;
        for (size_t idx = 0; idx < id_map_.size(); idx++) {
            try {
                Passage p = passages_.get(id_map_[idx]);
                if (filter && !filter->matches(p.metadata)) continue;
                texts.push_back(p.text);
                valid.push_back(idx);
            } catch (...) { continue; }
        }
        if (texts.empty()) return {};
        const size_t d = dimensions_, n = texts.size();
        std::vector<float> all(n * d);
        for (size_t b0 = 0; b0 < n; b0 += 100) { // batch_size = 100
            std::vector<std::string> batch(texts.begin() + b0, texts.begin() + std::min(n, b0 + 100));
            auto emb = provider.embed(batch);
            for (size_t i = 0; i < emb.size(); i++) std::copy(emb[i].begin(), emb[i].end(), all.begin() + (b0 + i) * d);
        }
        // scores + stable sort desc + take(k) on the device
        int ndev = 0;
        leann_device_count(&ndev);
        if (ndev < 1) throw Error("no HIP device visible. This library has no CPU fallback.");
        const size_t ld = (d + 3) & ~(size_t)3, k = std::min(top_k, n);
        void *dX = nullptr, *dQ = nullptr, *dK = nullptr, *dS = nullptr, *dC = nullptr;
        check(leann_device_malloc(0, n * ld * 4, &dX));
        check(leann_device_malloc(0, ld * 4, &dQ));
        check(leann_device_malloc(0, std::max<size_t>(k, 1) * 8, &dK));
        check(leann_device_malloc(0, std::max<size_t>(k, 1) * 4, &dS));
        check(leann_device_malloc(0, 4, &dC));
        std::vector<float> padded(n * ld, 0.0f), qp(ld, 0.0f);
        for (size_t i = 0; i < n; i++) std::copy(all.begin() + i * d, all.begin() + (i + 1) * d, padded.begin() + i * ld);
        std::copy(query_embedding.begin(), query_embedding.begin() + std::min(d, query_embedding.size()), qp.begin());
        check(leann_device_upload(dX, padded.data(), n * ld * 4));
        check(leann_device_upload(dQ, qp.data(), ld * 4));
        std::vector<uint64_t> keys(std::max<size_t>(k, 1));
        std::vector<float> scores(std::max<size_t>(k, 1));
        uint32_t cnt = 0;
        if (k > 0) {
            check(leann_scan_topk_device((const float *)dX, n, d, ld, (const float *)dQ, 1, k, nullptr, 0, (uint64_t *)dK, (float *)dS,
                                         (uint32_t *)dC, nullptr));
            check(leann_device_download(keys.data(), dK, k * 8));
            check(leann_device_download(scores.data(), dS, k * 4));
            check(leann_device_download(&cnt, dC, 4));
        }
        for (void *p : {dX, dQ, dK, dS, dC}) leann_device_free(p);
        std::vector<SearchResult> results;
        for (uint32_t i = 0; i < cnt; i++) {
            const std::string &id = id_map_[valid[keys[i]]];
            try {
                Passage p = passages_.get(id);
                results.push_back({id, scores[i], p.text, p.metadata}); // score = raw dot (recompute.rs:99)
            } catch (...) {}
        }
        return results;
    }
    size_t len() const { return id_map_.size(); }
    bool is_empty() const { return id_map_.empty(); }

  private:
    PassageStore passages_;
    std::vector<std::string> id_map_;
    size_t dimensions_ = 0;
};

} // namespace leann
