// search_plan_selftest — which beam-search kernel a call runs (csrc/search_plan.h) on the CPU: no GPU, no library.
//   no argument: plans every point of a grid of shapes, calls and knobs and checks the invariants below; one JSON line, exit status 1
//                on any violation.
//   --plans:     reads one case per line from stdin, "ld d feat_h bf16 maxdeg screen_ready nq k ef filtered build hash_bits nw no_feat256",
//                and prints one JSON line per case: what tests/test_cpu_search_plan.py holds to its hand-written rows.  An optional
//                fifteenth column "i8" (default 0) plans for int8 rows (tests/test_cpu_i8_rows.py).
#include "../csrc/search_plan.h"
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>

static const char *family_name(int f) {
    static const char *const names[] = {"F32", "SCREEN", "BF16", "FEAT", "FEAT256", "I8"};
    return f >= 0 && f < 6 ? names[f] : "?";
}

// "name<a, b, ..>" back into the fields of a plan that name a kernel; false: not a traversal kernel's name
static bool parse_name(const char *s, SearchPlan *out) {
    SearchPlan p = {};
    std::string base(s, strcspn(s, "<"));
    const char *args = s + base.size();
    if (*args != '<') return false;
    if (base.compare(0, 5, "wide_") == 0) { p.wide = true; base.erase(0, 5); }
    int nargs;
    if (base == "beam_search_kernel") { p.family = SEARCH_F32; nargs = 4; }
    else if (base == "beam_search_filtered_kernel") { p.family = SEARCH_F32; p.filtered = true; nargs = 3; }
    else if (base == "beam_search_screen_kernel") { p.family = SEARCH_SCREEN; nargs = 2; }
    else if (base == "bf16_beam_search_kernel") { p.family = SEARCH_BF16; nargs = 3; }
    else if (base == "bf16_beam_search_filtered_kernel") { p.family = SEARCH_BF16; p.filtered = true; nargs = 3; }
    else if (base == "beam_search_feat_kernel") { p.family = SEARCH_FEAT; nargs = 3; }
    else if (base == "beam_search_feat_filtered_kernel") { p.family = SEARCH_FEAT; p.filtered = true; nargs = 3; }
    else if (base == "beam_search_feat256_kernel") { p.family = SEARCH_FEAT256; nargs = 2; }
    else if (base == "beam_search_feat256_filtered_kernel") { p.family = SEARCH_FEAT256; p.filtered = true; nargs = 2; }
    else return false;
    long v[4] = {0, 0, 0, 0};
    const char *c = args + 1;
    for (int i = 0; i < nargs; i++) {
        if (i == 3) { // the BUILD switch of the plain kernel
            if (strncmp(c, "true", 4) == 0) { v[3] = 1; c += 4; }
            else if (strncmp(c, "false", 5) == 0) c += 5;
            else return false;
        } else {
            char *end;
            v[i] = strtol(c, &end, 10);
            if (end == c) return false;
            c = end;
        }
        if (i + 1 < nargs) {
            if (c[0] != ',' || c[1] != ' ') return false;
            c += 2;
        }
    }
    if (c[0] != '>' || c[1] != 0) return false;
    if (p.family == SEARCH_SCREEN) { p.T = (int)v[0]; p.R = (int)v[1]; p.NW = 4; }
    else if (p.family == SEARCH_FEAT256) { p.T = 1; p.R = (int)v[0]; p.NW = (int)v[1]; }
    else { p.T = (int)v[0]; p.R = (int)v[1]; p.NW = (int)v[2]; p.build = v[3] != 0; }
    *out = p;
    return true;
}

static int print_plans() {
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        unsigned ld, d, feat_h, bf16, maxdeg, screen, nq, k, ef, filtered, build, no_feat256, i8 = 0;
        int hash_bits, nw;
        if (sscanf(line, "%u %u %u %u %u %u %u %u %u %u %u %d %d %u %u", &ld, &d, &feat_h, &bf16, &maxdeg, &screen, &nq, &k, &ef, &filtered, &build,
                   &hash_bits, &nw, &no_feat256, &i8) < 14) {
            fprintf(stderr, "search_plan_selftest: bad case line: %s", line);
            return 2;
        }
        SearchShape s = {};
        s.ld = ld; s.d = d; s.feat_h = feat_h; s.bf16 = bf16 != 0; s.maxdeg = maxdeg; s.screen_ready = screen != 0;
        s.i8 = i8 != 0;
        const SearchCall c = {nq, k, ef, filtered != 0, build != 0};
        const SearchKnobs kn = {hash_bits, nw, no_feat256 != 0};
        const SearchPlan p = search_plan(s, c, kn);
        char name[96] = "";
        if (!p.err) search_plan_name(p, name, sizeof name);
        printf("{\"err\": %d, \"msg\": \"%s\", \"family\": \"%s\", \"name\": \"%s\", \"hash_bits\": %u, \"lds_bytes\": %zu}\n", p.err, p.msg,
               p.err ? "" : family_name(p.family), name, p.hash_bits, p.lds_bytes);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1) return strcmp(argv[1], "--plans") == 0 ? print_plans() : 2;
    const uint32_t nqs[] = {1, 384, 385, 512, 513, 640, 641, 4096}, efs[] = {1, 64, 65, 341, 342, 683, 5000}, degs[] = {16, 64, 65, 128};
    const SearchKnobs knobs[] = {{0, 0, false}, {8, 0, false}, {0, 1, false}, {0, 8, false}, {0, 16, false}, {0, 0, true}};
    long cases = 0, accepted = 0, refused_build = 0, refused_width = 0, refused_lds = 0;
    long bad_family = 0, bad_lds = 0, bad_limit = 0, bad_nw = 0, bad_nbuf = 0, bad_screen = 0, bad_wide = 0, bad_hash = 0, bad_width = 0, bad_name = 0,
         bad_refusal = 0;
    std::set<uint64_t> named;
    // widths: stored rows (f32, then bf16) of every ld in 4..4100 step 4, then recompute-on rows of every feat_h in 1..1100
    for (int kind = 0; kind < 3; kind++) {
        const uint32_t w0 = kind < 2 ? 4 : 1, w1 = kind < 2 ? 4100 : 1100, step = kind < 2 ? 4 : 1;
        for (uint32_t w = w0; w <= w1; w += step)
            for (uint32_t nq : nqs) for (uint32_t ef : efs) for (uint32_t deg : degs) for (int flags = 0; flags < 8; flags++) for (const SearchKnobs &kn : knobs) {
                SearchShape s = {};
                s.ld = kind < 2 ? w : 768; s.d = s.ld; s.feat_h = kind == 2 ? w : 0; s.bf16 = kind == 1; s.maxdeg = deg;
                s.screen_ready = (flags & 4) != 0;
                const SearchCall c = {nq, ef < 10 ? ef : 10, ef, (flags & 1) != 0, (flags & 2) != 0};
                const SearchPlan p = search_plan(s, c, kn);
                cases++;
                const uint32_t width = kind < 2 ? s.ld : s.feat_h;
                if (p.err) {
                    if ((p.err != SEARCH_PLAN_INVALID && p.err != SEARCH_PLAN_UNSUPPORTED) || !p.msg[0]) bad_refusal++;
                    if (p.err == SEARCH_PLAN_UNSUPPORTED) { // construction searches of bf16 and recompute-on rows, nothing else
                        refused_build++;
                        if (!c.build || kind == 0) bad_refusal++;
                    } else if (p.lds_bytes) { // the LDS figure is the last thing a plan computes
                        refused_lds++;
                        if (p.lds_bytes <= LEANN_SEARCH_LDS_LIMIT) bad_refusal++;
                    } else {
                        refused_width++;
                        if (width <= (kind < 2 ? 4096u : 1024u)) bad_refusal++;
                    }
                    continue;
                }
                accepted++;
                if (c.build && kind != 0) bad_refusal++;
                if (kind == 0 ? (p.family != SEARCH_F32 && p.family != SEARCH_SCREEN)
                              : kind == 1 ? p.family != SEARCH_BF16 : (p.family != SEARCH_FEAT && p.family != SEARCH_FEAT256))
                    bad_family++;
                if (p.family == SEARCH_FEAT256 && (s.feat_h != 256 || kn.no_feat256)) bad_family++;
                if (p.lds_bytes > LEANN_SEARCH_LDS_LIMIT) bad_limit++;
                if (p.NW != 4 && p.NW != 8 && p.NW != 16) bad_nw++;
                if (p.filtered != c.filtered || (p.build && (!c.build || c.filtered))) bad_family++;
                // the hop loop's form follows the wave count: per-parity buffers (nbuf = 2) iff NW > 4
                const uint32_t kf = p.filtered ? c.k : 0u;
                if (p.lds_bytes != search_lds_bytes(c.ef, s.maxdeg, p.hash_bits, kf, p.NW > 4 ? 2u : 1u)) bad_lds++;
                if (p.lds_bytes == search_lds_bytes(c.ef, s.maxdeg, p.hash_bits, kf, p.NW > 4 ? 1u : 2u)) bad_nbuf++;
                const bool screen_ok = p.NW == 4 && (p.T == 3 || p.T == 6) && s.screen_ready && !c.filtered && !c.build && s.maxdeg <= 64;
                if ((p.family == SEARCH_SCREEN) != (kind == 0 && screen_ok)) bad_screen++;
                if (p.wide != (s.maxdeg > 64) || (p.wide && p.NW == 8)) bad_wide++;
                if (p.hash_bits < 6 || p.hash_bits > 15) bad_hash++;
                if (p.T < 1 || p.R < 1 || (uint32_t)p.T * 256u < width) bad_width++;
                // the name is a function of the seven fields that name a kernel: checked once per distinct set of them
                SearchPlan key = {};
                key.family = p.family; key.T = p.T; key.R = p.R; key.NW = p.NW; key.wide = p.wide; key.filtered = p.filtered; key.build = p.build;
                const uint64_t packed = ((((uint64_t)key.family << 16 | (uint64_t)key.T) << 16 | (uint64_t)key.R) << 16 | (uint64_t)key.NW) << 3 |
                                        (uint64_t)(key.wide << 2 | key.filtered << 1 | key.build);
                if (!named.insert(packed).second) continue;
                char name[96];
                SearchPlan q;
                const int len = search_plan_name(key, name, sizeof name);
                if (len <= 0 || len >= (int)sizeof name || !parse_name(name, &q) || q.family != p.family || q.T != p.T || q.R != p.R || q.NW != p.NW ||
                    q.wide != p.wide || q.filtered != p.filtered || q.build != p.build)
                    bad_name++;
            }
    }
    const long bad = bad_family + bad_lds + bad_limit + bad_nw + bad_nbuf + bad_screen + bad_wide + bad_hash + bad_width + bad_name + bad_refusal;
    printf("{\"cases\": %ld, \"accepted\": %ld, \"refused_build\": %ld, \"refused_width\": %ld, \"refused_lds\": %ld, \"bad_family\": %ld, "
           "\"bad_lds\": %ld, \"bad_limit\": %ld, \"bad_nw\": %ld, \"bad_nbuf\": %ld, \"bad_screen\": %ld, \"bad_wide\": %ld, \"bad_hash\": %ld, "
           "\"bad_width\": %ld, \"bad_name\": %ld, \"bad_refusal\": %ld, \"kernels\": %zu}\n",
           cases, accepted, refused_build, refused_width, refused_lds, bad_family, bad_lds, bad_limit, bad_nw, bad_nbuf, bad_screen, bad_wide,
           bad_hash, bad_width, bad_name, bad_refusal, named.size());
    return bad ? 1 : 0;
}
