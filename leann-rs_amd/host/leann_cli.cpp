// leann_cli.cpp — `leann search` with the reference's flags and output formats (src/cli/search.rs:10-260),
// plus a minimal `leann build` over a passages JSONL so that an index directory can be produced offline
// (the reference's ingestion — file walking, chunking, HTTP embedding — is out of scope).
//
// Additive, because every real embedding provider needs the network (src/cli/search.rs:100-112):
//     --embedding-mode synthetic     deterministic hashed-token embedder (leann_host.hpp)
//     --query-vector-file FILE       raw little-endian f32[dims] query embedding
//     --device N                     HIP device ordinal
#include "leann_host.hpp"

#include <cstring>
#include <iostream>
#include <unistd.h>

using namespace leann;

struct SearchArgs {
    std::string query;
    std::optional<std::string> index;
    size_t top_k = 5, complexity = 64;
    bool show_metadata = false, hybrid = false, auto_hybrid = true, expand = true;
    std::optional<std::string> filter;
    float hybrid_alpha = 0.7f;
    bool compat_polarity = true; // additive: SURVEY.md N1 (see SearchOptions::compat_polarity)
    std::string format = "text";
    std::optional<std::string> query_prompt_template, embedding_mode, query_vector_file;
    std::string device = getenv("LEANN_DEVICES") ? getenv("LEANN_DEVICES") : "0"; // "0", or a list / range = sharded (leann_backend.h)
    bool device_filter = false;
    bool bm25_device = true;
    bool hybrid_filter_inside = false;
    std::optional<std::string> queries_file;
    size_t refine = 0;           // additive: --refine <FETCH_K> (SearchOptions::refine_fetch_k)
    bool refine_rows_host = true;
};

static void usage_search() {
    puts("Query an index\n\nUsage: leann search [OPTIONS] <QUERY>\n\nArguments:\n  <QUERY>  Search query\n\nOptions:\n"
         "  -i, --index <INDEX>                Index name to search (defaults to current directory name)\n"
         "      --top-k <TOP_K>                Number of results to return [default: 5]\n"
         "      --complexity <COMPLEXITY>      Search complexity (higher = more accurate but slower) [default: 64]\n"
         "      --show-metadata                Show file paths in results\n"
         "  -f, --filter <FILTER>              Filter results by metadata (e.g., \"source:*.rs\" or \"type=code\")\n"
         "      --hybrid                       Enable hybrid search (vector + BM25)\n"
         "      --auto-hybrid <AUTO_HYBRID>    Auto-enable hybrid search for short queries (1-3 words) [default: true]\n"
         "      --expand <EXPAND>              Expand short queries with related terms for better recall [default: true]\n"
         "      --hybrid-alpha <HYBRID_ALPHA>  Weight for vector scores in hybrid mode (0.0-1.0, default 0.7) [default: 0.7]\n"
         "      --format <FORMAT>              Output format (text, json) [default: text] [possible values: text, json]\n"
         "      --embedding-api-key <KEY>      API key for embedding service [env: OPENAI_API_KEY]\n"
         "      --embedding-api-base <URL>     OpenAI API base URL [env: OPENAI_BASE_URL]\n"
         "      --embedding-host <HOST>        Ollama host for embeddings [env: OLLAMA_HOST]\n"
         "      --query-prompt-template <T>    Query prompt template prefix for asymmetric embedding models\n"
         "      --embedding-mode <MODE>        (additive) override the index's embedding mode; `synthetic` works offline\n"
         "      --query-vector-file <FILE>     (additive) raw f32 query embedding instead of embedding the query text\n"
         "      --device <SPEC>                (additive) HIP device ordinal, or a list / range (\"0-7\") = index sharded over several GPUs [env: LEANN_DEVICES] [default: 0]\n"
         "      --device-filter                (additive) evaluate --filter inside the GPU traversal instead of 5x over-fetch + post-filter\n"
         "      --queries-file <FILE>          (additive) one query per line instead of <QUERY>: the batch is searched in one backend call and,\n"
         "                                     with --hybrid, one device BM25 + rerank call; prints a JSON array with one result array per query\n"
         "      --bm25 <WHERE>                 (additive) where hybrid mode scores BM25: device (inverted index in HBM) or host; same output [default: device] [possible values: device, host]\n"
         "      --hybrid-filter <WHEN>         (additive) hybrid mode: inside = BM25 and its rerank see only what --device-filter allows and no removed passage; post = filter after the rerank [default: post] [possible values: inside, post]\n"
         "      --refine <FETCH_K>             (additive) fetch FETCH_K candidates from the walk and score them again on the exact f32 rows of\n"
         "                                     documents.embeddings (`leann build --recompute`): an int8 / bf16 index then prints an f32 index's scores;\n"
         "                                     not with --hybrid (short queries are not switched to hybrid either)\n"
         "      --refine-rows <WHERE>          (additive) where --refine keeps the exact rows: host (pinned memory read across the bus) or hbm [default: host] [possible values: hbm, host]\n"
         "  -h, --help                         Print help");
}

static bool parse_bool(const std::string &v) {
    if (v == "true") return true;
    if (v == "false") return false;
    throw Error("invalid value '" + v + "' for bool flag (expected true|false)");
}

static int run_search(int argc, char **argv) {
    SearchArgs a;
    bool have_query = false;
    for (int i = 0; i < argc; i++) {
        std::string s = argv[i];
        auto val = [&]() -> std::string {
            size_t eq = s.find('=');
            if (s.rfind("--", 0) == 0 && eq != std::string::npos) return s.substr(eq + 1);
            if (i + 1 >= argc) throw Error("a value is required for '" + s + "' but none was supplied");
            return argv[++i];
        };
        std::string name = s.rfind("--", 0) == 0 ? s.substr(0, s.find('=')) : s;
        if (name == "-h" || name == "--help") { usage_search(); return 0; }
        else if (name == "-i" || name == "--index") a.index = val();
        else if (name == "--top-k") a.top_k = std::stoul(val());
        else if (name == "--complexity") a.complexity = std::stoul(val());
        else if (name == "--show-metadata") a.show_metadata = true;
        else if (name == "--device-filter") a.device_filter = true;
        else if (name == "-f" || name == "--filter") a.filter = val();
        else if (name == "--hybrid") a.hybrid = true;
        else if (name == "--auto-hybrid") a.auto_hybrid = parse_bool(val());
        else if (name == "--expand") a.expand = parse_bool(val());
        else if (name == "--hybrid-alpha") a.hybrid_alpha = std::stof(val());
        else if (name == "--compat-polarity") a.compat_polarity = parse_bool(val());
        else if (name == "--format") { a.format = val(); if (a.format != "text" && a.format != "json") throw Error("invalid value '" + a.format + "' for '--format <FORMAT>' [possible values: text, json]"); }
        else if (name == "--embedding-api-key" || name == "--embedding-api-base" || name == "--embedding-host") (void)val();
        else if (name == "--query-prompt-template") a.query_prompt_template = val();
        else if (name == "--embedding-mode") a.embedding_mode = val();
        else if (name == "--query-vector-file") a.query_vector_file = val();
        else if (name == "--device") a.device = val();
        else if (name == "--queries-file") a.queries_file = val();
        else if (name == "--bm25") { std::string w = val(); if (w != "device" && w != "host") throw Error("invalid value '" + w + "' for '--bm25 <WHERE>' [possible values: device, host]"); a.bm25_device = w == "device"; }
        else if (name == "--hybrid-filter") { std::string w = val(); if (w != "inside" && w != "post") throw Error("invalid value '" + w + "' for '--hybrid-filter <WHEN>' [possible values: inside, post]"); a.hybrid_filter_inside = w == "inside"; }
        else if (name == "--refine") { a.refine = std::stoul(val()); if (a.refine == 0) throw Error("invalid value '0' for '--refine <FETCH_K>': at least 1"); }
        else if (name == "--refine-rows") { std::string w = val(); if (w != "hbm" && w != "host") throw Error("invalid value '" + w + "' for '--refine-rows <WHERE>' [possible values: hbm, host]"); a.refine_rows_host = w == "host"; }
        else if (name == "-v" || name == "--verbose" || name == "-q" || name == "--quiet") {}
        else if (!s.empty() && s[0] == '-' && s.size() > 1) throw Error("unexpected argument '" + s + "' found");
        else if (!have_query) { a.query = s; have_query = true; }
        else throw Error("unexpected argument '" + s + "' found");
    }
    if (!have_query && !a.queries_file) throw Error("the following required arguments were not provided:\n  <QUERY>");
    if (a.refine && a.hybrid)
        throw Error("--refine together with --hybrid is not supported: the hybrid rerank blends the walk's distances, and refining inside it "
                    "is a follow-up; drop one of the two");

    // search.rs:75-88
    std::string index_name;
    if (a.index) index_name = *a.index;
    else {
        char cwd[4096];
        std::string d = getcwd(cwd, sizeof cwd) ? cwd : "index";
        size_t sl = d.find_last_of('/');
        index_name = sl == std::string::npos ? d : d.substr(sl + 1);
        if (index_name.empty()) index_name = "index";
    }
    std::string index_dir = find_index(index_name);
    std::string meta_path = index_dir + "/documents.leann.meta.json", index_path = index_dir + "/documents.leann";
    IndexMeta meta = IndexMeta::load(meta_path);
    const bool is_pruned = meta.is_pruned;

    std::string mode = a.embedding_mode ? *a.embedding_mode : meta.embedding_mode;
    std::string query_template = a.query_prompt_template.value_or("");
    if (!a.query_prompt_template && !meta.embedding_options.is_null())
        if (auto *t = meta.embedding_options.get("query_prompt_template"))
            if (t->is_string()) query_template = t->s;

    std::optional<MetadataFilter> filter;
    if (a.filter) {
        filter = MetadataFilter::parse(*a.filter);
        if (!filter) throw Error("Invalid filter syntax: " + *a.filter);
    }
    size_t word_count = 0;
    { std::istringstream ws(a.query); for (std::string w; ws >> w;) word_count++; }
    const bool use_hybrid = a.hybrid || (a.auto_hybrid && word_count <= 3 && !a.refine); // search.rs:147-148 (--refine: never switched on by itself)

    auto embed_query = [&](const std::string &text) -> std::vector<float> {
        if (a.query_vector_file) {
            std::string raw = read_file(*a.query_vector_file);
            if (raw.size() != meta.dimensions * 4) throw Error("--query-vector-file must hold " + std::to_string(meta.dimensions) + " f32 values");
            std::vector<float> v(meta.dimensions);
            memcpy(v.data(), raw.data(), raw.size());
            return v;
        }
        if (mode != "synthetic" && mode != "synthetic-linear") {
            if (mode == "openai" || mode == "ollama" || mode == "gemini")
                throw Error("Embedding mode '" + mode + "' needs a network service that is unavailable in this build; "
                            "pass --embedding-mode synthetic or --query-vector-file");
            throw Error("Unknown embedding mode in index: " + mode); // search.rs:112
        }
        return EmbeddingProvider(mode, meta.dimensions).embed_with_template({text}, query_template)[0];
    };

    auto results_json = [](const std::vector<SearchResult> &rs) { // search.rs:211-223
        lj::Value arr = lj::Value::array();
        for (auto &r : rs) {
            lj::Value o = lj::Value::object();
            o["id"] = lj::Value::string(r.id);
            o["score"] = lj::Value::number((double)r.score); // f32 widened, like serde_json's From<f32>
            o["text"] = lj::Value::string(r.text);
            o["metadata"] = r.metadata;
            arr.a->push_back(o);
        }
        return arr;
    };
    if (a.queries_file) { // additive: IndexSearcher::search_batch_with_options; hybrid mode is what --hybrid says, for every query
        if (is_pruned) throw Error("--queries-file needs an index with an ANN graph (not a pruned one)");
        std::vector<std::string> texts;
        {
            std::istringstream ss(read_file(*a.queries_file));
            for (std::string line; std::getline(ss, line);) {
                if (!line.empty() && line.back() == '\r') line.pop_back();
                texts.push_back(line);
            }
        }
        IndexSearcher searcher = IndexSearcher::load(index_path, meta, a.device.c_str());
        std::vector<std::vector<float>> embeddings;
        for (auto &t : texts) embeddings.push_back(embed_query(t));
        SearchOptions opts(a.top_k, a.complexity);
        if (filter) opts.with_filter(*filter);
        if (filter && a.device_filter) opts.with_device_filter(*a.filter);
        if (a.hybrid) opts.with_hybrid("", a.hybrid_alpha);
        if (a.refine) opts.with_refine(a.refine, a.refine_rows_host);
        opts.with_compat_polarity(a.compat_polarity).with_bm25_device(a.bm25_device).with_hybrid_filter_inside(a.hybrid_filter_inside);
        lj::Value all = lj::Value::array();
        for (auto &rs : searcher.search_batch_with_options(embeddings, texts, opts)) all.a->push_back(results_json(rs));
        printf("%s\n", lj::to_string_pretty(all).c_str());
        return 0;
    }

    std::vector<SearchResult> results;
    auto graph_search = [&]() {
        IndexSearcher searcher = IndexSearcher::load(index_path, meta, a.device.c_str());
        // query expansion (src/index/query.rs) is a text heuristic outside the scoped path: not applied
        auto q = embed_query(a.query);
        SearchOptions opts(a.top_k, a.complexity);
        if (filter) opts.with_filter(*filter);
        if (filter && a.device_filter) opts.with_device_filter(*a.filter);
        if (use_hybrid) opts.with_hybrid(a.query, a.hybrid_alpha);
        if (a.refine) opts.with_refine(a.refine, a.refine_rows_host);
        opts.with_compat_polarity(a.compat_polarity).with_bm25_device(a.bm25_device).with_hybrid_filter_inside(a.hybrid_filter_inside);
        results = searcher.search_with_options(q, opts);
    };
    // A pruned index (search.rs:151-167) recomputes embeddings at query time.  The reference scans every passage through the provider
    // (RecomputeSearcher).  When the directory holds a recompute-on GRAPH (`leann build --recompute-graph`: our file format version 2 —
    // graph + compact encoder inputs, no vectors) the graph is walked instead and distances are recomputed on the device per visited node.
    const std::string ann_file = with_extension(index_path, meta.backend_name == "diskann" ? "diskann" : "index");
    bool pruned_graph = false;
    if (is_pruned && file_exists(ann_file)) {
        std::ifstream f(ann_file, std::ios::binary);
        char hd[16] = {0};
        f.read(hd, 16);
        uint32_t version = 0;
        memcpy(&version, hd + 8, 4);
        pruned_graph = f.gcount() == 16 && !memcmp(hd, "LEANNGX1", 8) && version == 2;
    }
    if (is_pruned && !pruned_graph) {
        auto q = embed_query(a.query);
        if (mode != "synthetic" && mode != "synthetic-linear")
            throw Error("recompute mode needs an embedding provider; only `synthetic` / `synthetic-linear` work offline");
        EmbeddingProvider provider(mode, meta.dimensions);
        RecomputeSearcher searcher = RecomputeSearcher::load(index_path, meta.dimensions);
        results = searcher.search(q, provider, a.top_k, filter ? &*filter : nullptr);
    } else {
        graph_search();
    }

    if (a.format == "json") {
        printf("%s\n", lj::to_string_pretty(results_json(results)).c_str());
    } else { // search.rs:225-256
        printf("\nSearch results for '%s' (top %zu):\n\n", a.query.c_str(), results.size());
        for (size_t i = 0; i < results.size(); i++) {
            auto &r = results[i];
            printf("%zu. Score: %.4f\n", i + 1, (double)r.score);
            if (a.show_metadata) {
                if (auto *src = r.metadata.get("source")) printf("   Source: %s\n", lj::to_string(*src).c_str());
                if (r.metadata.is_object())
                    for (auto &kv : *r.metadata.o)
                        if (kv.first != "source") printf("   %s: %s\n", kv.first.c_str(), lj::to_string(kv.second).c_str());
            }
            std::string text = r.text;
            if (text.size() > 200) { // truncate on a UTF-8 boundary
                size_t end = 200;
                while (end > 0 && ((unsigned char)text[end] & 0xC0) == 0x80) end--;
                text = text.substr(0, end) + "...";
            }
            printf("   %s\n\n", text.c_str());
        }
    }
    return 0;
}

// leann build --index-dir DIR --passages-jsonl FILE [--backend-name hnsw|diskann] [--graph-degree 32]
//             [--complexity 64] [--dimensions 128] [--embedding-mode synthetic|synthetic-linear] [--recompute] [--pruned]
//             [--recompute-graph] [--row-type f32|bf16|int8]
// --recompute       also write documents.embeddings (only in recompute mode, src/index/builder.rs:105-113), so that the index can be
//                   pruned later; off by default like the reference (meta.is_recompute = args.recompute)
// --pruned          no ANN file and no embeddings: the reference's pruned state (brute-force recompute at query time)
// --recompute-graph (needs --embedding-mode synthetic-linear) graph + compact encoder inputs, no vectors
// --row-type        what the ANN file stores per element: f32 (default) or bf16 (half the file and device memory; the rows are rounded
//                   first and the graph is built on the rounded rows, DESIGN.md "bf16 rows") or int8 (a quarter: one power-of-two
//                   scale per column and 8-bit codes, the graph built on the dequantised rows, DESIGN.md "int8 rows")
static const char *row_type_name(int row_type) { return row_type == LEANN_ROWS_BF16 ? "bf16" : row_type == LEANN_ROWS_I8 ? "int8" : "f32"; }
static int parse_row_type(const std::string &v) {
    if (v == "f32") return LEANN_ROWS_F32;
    if (v == "bf16") return LEANN_ROWS_BF16;
    if (v == "int8") return LEANN_ROWS_I8;
    throw Error("invalid value '" + v + "' for '--row-type': expected f32 or bf16, or int8");
}
static int run_build(int argc, char **argv) {
    std::string dir, jsonl, backend_name = "hnsw", mode = "synthetic";
    size_t degree = 32, complexity = 64, dims = 128;
    bool pruned = false, recompute = false, rgraph = false; // is_recompute = args.recompute, default false (src/cli/build.rs:363)
    int row_type = LEANN_ROWS_F32;
    for (int i = 0; i < argc; i++) {
        std::string s = argv[i];
        auto val = [&]() -> std::string { if (i + 1 >= argc) throw Error("missing value for " + s); return argv[++i]; };
        if (s == "--index-dir") dir = val();
        else if (s == "--passages-jsonl" || s == "--docs") jsonl = val();
        else if (s == "--backend-name") backend_name = val();
        else if (s == "--graph-degree") degree = std::stoul(val());
        else if (s == "--complexity") complexity = std::stoul(val());
        else if (s == "--dimensions") dims = std::stoul(val());
        else if (s == "--embedding-mode") mode = val();
        else if (s == "--pruned") pruned = true;
        else if (s == "--recompute") recompute = true;
        else if (s == "--recompute-graph") { rgraph = true; mode = "synthetic-linear"; }
        else if (s == "--row-type") row_type = parse_row_type(val());
        else throw Error("unexpected argument '" + s + "' found");
    }
    if (dir.empty() || jsonl.empty()) throw Error("usage: leann build --index-dir DIR --passages-jsonl FILE [...]");
    int backend = backend_name == "hnsw" ? LEANN_BACKEND_HNSW : backend_name == "diskann" ? LEANN_BACKEND_DISKANN : -1;
    if (backend < 0) throw Error("Unknown backend: " + backend_name);
    if (row_type != LEANN_ROWS_F32 && (pruned || rgraph)) throw Error("--row-type applies to an index of stored vectors, not to --pruned / --recompute-graph");
    EmbeddingProvider provider(mode, dims);
    ::mkdir(dir.c_str(), 0755);
    std::string stem = dir + "/documents.leann";
    std::ifstream in(jsonl);
    if (!in) throw Error("cannot open " + jsonl);
    PassageStoreWriter w(stem);
    std::vector<float> all;
    std::vector<uint16_t> feats;
    std::ofstream ids(with_extension(stem, "ids.txt"));
    size_t n = 0;
    for (std::string line; std::getline(in, line);) {
        if (line.empty()) continue;
        lj::Value v = lj::parse(line);
        Passage p;
        p.id = v.get("id") ? v.get("id")->s : std::to_string(n + 1); // chunk ids start at "1" (chunker/simple.rs:38-40)
        p.text = v.get("text") ? v.get("text")->s : "";
        p.metadata = v.get("metadata") ? *v.get("metadata") : lj::Value::object();
        w.add(p);
        ids << p.id << "\n";
        if (rgraph) {
            auto f = linear_features(p.text);
            feats.insert(feats.end(), f.begin(), f.end());
        } else if (!pruned) {
            auto e = provider.embed({p.text})[0];
            all.insert(all.end(), e.begin(), e.end());
        }
        n++;
    }
    w.finish();
    ids.close();
    if (rgraph) {
        // the embeddings exist only transiently on the device while the graph is built (leann_recompute_build_index)
        leann_recompute *r = nullptr;
        check(leann_recompute_create_host(feats.data(), n, LINEAR_H, provider.weights().data(), dims, 0, 0, &r));
        leann_backend *h = nullptr;
        int rc = leann_recompute_build_index(r, backend, degree, complexity, &h);
        if (rc == 0) rc = leann_backend_save(h, stem.c_str());
        if (h) leann_backend_close(h);
        leann_recompute_close(r);
        check(rc);
    } else if (!pruned) {
        if (recompute) { // src/index/embeddings.rs: raw LE f32 [n x dims]
            std::ofstream ef(with_extension(stem, "embeddings"), std::ios::binary);
            ef.write((const char *)all.data(), (std::streamsize)(all.size() * 4));
        }
        if (row_type == LEANN_ROWS_F32) check(leann_backend_build(backend, all.data(), n, dims, degree, complexity, stem.c_str()));
        else check(leann_backend_build_rows(backend, all.data(), n, dims, degree, complexity, row_type, stem.c_str()));
    }
    IndexMeta m;
    m.version = "1.0";
    m.backend_name = backend_name;
    m.embedding_model = mode == "synthetic" ? "synthetic-hash" : "synthetic-linear-256";
    m.embedding_mode = mode;
    m.dimensions = dims;
    m.passage_count = n;
    m.is_recompute = pruned || rgraph || recompute;
    m.is_pruned = pruned || rgraph;
    if (rgraph) {
        m.backend_kwargs = lj::Value::object();
        m.backend_kwargs["recompute_graph"] = lj::Value::boolean(true);
        m.backend_kwargs["feature_dim"] = lj::Value::integer((int64_t)LINEAR_H);
    }
    m.save(dir + "/documents.leann.meta.json");
    printf("Indexed %zu passages (%zu dims, backend %s%s) into %s\n", n, dims, backend_name.c_str(),
           rgraph ? ", recompute-on graph (no vectors)" : pruned ? ", pruned" : row_type == LEANN_ROWS_BF16 ? ", bf16 rows" : row_type == LEANN_ROWS_I8 ? ", int8 rows" : "", dir.c_str());
    return 0;
}

// leann delete <index> --ids a,b,c | --ids-file F   (additive; the reference can only append)
// Passage ids are mapped to positions through ids.txt and removed from the ANN index (leann_backend_remove_from_index: tombstones +
// graph repair, persisted beside the index file).  The passages, ids and meta files are not rewritten: positions keep their numbers.
static int run_delete(int argc, char **argv) {
    std::string index_name, device;
    std::vector<std::string> ids;
    auto add_ids = [&](const std::string &text, char sep) {
        std::istringstream ss(text);
        for (std::string t; std::getline(ss, t, sep);) {
            if (!t.empty() && t.back() == '\r') t.pop_back();
            if (!t.empty()) ids.push_back(t);
        }
    };
    for (int i = 0; i < argc; i++) {
        std::string s = argv[i];
        auto val = [&]() -> std::string { if (i + 1 >= argc) throw Error("a value is required for '" + s + "' but none was supplied"); return argv[++i]; };
        if (s == "-h" || s == "--help") { puts("Remove passages from an index\n\nUsage: leann delete <INDEX> --ids a,b,c | --ids-file <FILE>"); return 0; }
        else if (s == "--ids") add_ids(val(), ',');
        else if (s == "--ids-file") add_ids(read_file(val()), '\n');
        else if (s == "-i" || s == "--index") index_name = val();
        else if (!s.empty() && s[0] == '-' && s.size() > 1) throw Error("unexpected argument '" + s + "' found");
        else if (index_name.empty()) index_name = s;
        else throw Error("unexpected argument '" + s + "' found");
    }
    if (index_name.empty()) throw Error("the following required arguments were not provided:\n  <INDEX>");
    if (ids.empty()) throw Error("no passage ids given: pass --ids a,b,c or --ids-file <FILE>");
    std::string index_dir = find_index(index_name);
    std::string index_path = index_dir + "/documents.leann";
    IndexMeta meta = IndexMeta::load(index_path + ".meta.json");
    int backend = meta.backend_name == "hnsw" ? LEANN_BACKEND_HNSW : meta.backend_name == "diskann" ? LEANN_BACKEND_DISKANN : -1;
    if (backend < 0) throw Error("Unknown backend: " + meta.backend_name);
    PassageStore passages = PassageStore::open(index_path);
    std::vector<std::string> id_map = read_id_map(index_path, passages);
    std::unordered_map<std::string, uint64_t> pos;
    for (size_t i = 0; i < id_map.size(); i++) pos.emplace(id_map[i], (uint64_t)i);
    std::vector<uint64_t> keys;
    for (auto &id : ids) {
        auto it = pos.find(id);
        if (it == pos.end()) throw Error("unknown passage id '" + id + "' in index '" + index_name + "'");
        keys.push_back(it->second);
    }
    check(leann_backend_remove_from_index(backend, keys.data(), keys.size(), meta.dimensions, index_path.c_str()));
    leann_backend *h = nullptr;
    check(leann_backend_open(index_path.c_str(), backend, meta.dimensions, "0", &h));
    const size_t live = leann_backend_live_len(h);
    leann_backend_close(h);
    std::sort(keys.begin(), keys.end());
    const size_t distinct = (size_t)(std::unique(keys.begin(), keys.end()) - keys.begin());
    printf("Index '%s': removed %zu passages, %zu live\n", index_name.c_str(), distinct, live);
    return 0;
}

// leann convert <index> --row-type bf16|int8   (additive)
// Rewrites the ANN file of an existing f32 index with bf16 or int8 rows: open -> leann_backend_to_rows -> save.  The graph stays the one that
// was built on the exact rows; removals (the tombstone sidecar) are carried over.  Passages, ids and meta files are not touched: the
// row type lives in the index file alone.
static int run_convert(int argc, char **argv) {
    std::string index_name;
    int row_type = -1;
    for (int i = 0; i < argc; i++) {
        std::string s = argv[i];
        auto val = [&]() -> std::string { if (i + 1 >= argc) throw Error("a value is required for '" + s + "' but none was supplied"); return argv[++i]; };
        if (s == "-h" || s == "--help") { puts("Rewrite an index with another row type\n\nUsage: leann convert <INDEX> --row-type bf16|int8"); return 0; }
        else if (s == "--row-type") row_type = parse_row_type(val());
        else if (s == "-i" || s == "--index") index_name = val();
        else if (!s.empty() && s[0] == '-' && s.size() > 1) throw Error("unexpected argument '" + s + "' found");
        else if (index_name.empty()) index_name = s;
        else throw Error("unexpected argument '" + s + "' found");
    }
    if (index_name.empty()) throw Error("the following required arguments were not provided:\n  <INDEX>");
    if (row_type < 0) throw Error("the following required arguments were not provided:\n  --row-type <f32|bf16|int8>");
    std::string index_path = find_index(index_name) + "/documents.leann";
    IndexMeta meta = IndexMeta::load(index_path + ".meta.json");
    int backend = meta.backend_name == "hnsw" ? LEANN_BACKEND_HNSW : meta.backend_name == "diskann" ? LEANN_BACKEND_DISKANN : -1;
    if (backend < 0) throw Error("Unknown backend: " + meta.backend_name);
    leann_backend *h = nullptr, *b = nullptr;
    check(leann_backend_open(index_path.c_str(), backend, meta.dimensions, "0", &h));
    if (leann_backend_row_type(h) == row_type) {
        leann_backend_close(h);
        printf("Index '%s': rows are %s already\n", index_name.c_str(), row_type_name(row_type));
        return 0;
    }
    int rc = leann_backend_to_rows(h, row_type, &b);
    if (rc == 0) rc = leann_backend_save(b, index_path.c_str());
    const size_t n = leann_backend_len(h);
    if (b) leann_backend_close(b);
    leann_backend_close(h);
    check(rc);
    printf("Index '%s': %zu rows rewritten as %s\n", index_name.c_str(), n, row_type_name(row_type));
    return 0;
}

int main(int argc, char **argv) {
    try {
        if (argc < 2 || !strcmp(argv[1], "-h") || !strcmp(argv[1], "--help")) {
            puts("LEANN search path on MI355X\n\nUsage: leann <COMMAND>\n\nCommands:\n  search  Query an index\n  build   Build an index from a passages JSONL (synthetic embeddings)\n  delete  Remove passages from an index\n  convert Rewrite an index with another row type (f32 -> bf16, f32 -> int8)\n");
            return argc < 2 ? 2 : 0;
        }
        if (!strcmp(argv[1], "--version") || !strcmp(argv[1], "-V")) { printf("leann %s\n", leann_version()); return 0; }
        if (!strcmp(argv[1], "search")) return run_search(argc - 2, argv + 2);
        if (!strcmp(argv[1], "build")) return run_build(argc - 2, argv + 2);
        if (!strcmp(argv[1], "delete")) return run_delete(argc - 2, argv + 2);
        if (!strcmp(argv[1], "convert")) return run_convert(argc - 2, argv + 2);
        throw Error(std::string("unrecognized subcommand '") + argv[1] + "'");
    } catch (const std::exception &e) {
        fprintf(stderr, "Error: %s\n", e.what());
        return 1;
    }
}
