// topk_plan_selftest — how an exhaustive top-k cuts its rows into chunks and sizes its scratch (csrc/topk_plan.h) on the CPU: no GPU,
// no library.
//   no argument: plans every point of a grid of rows, queries and k, with the exact scan's and the recompute search's parameters,
//                emission wanted and not, and checks the invariants below; one JSON line, exit status 1 on any violation.
//   --plans:     reads one case per line from stdin, "scan|recompute emit n nq k", and prints one JSON line per case: what
//                tests/test_cpu_topk_plan.py holds to its hand-written rows.
#include "../csrc/topk_plan.h"
#include <cstdio>
#include <cstring>

static const size_t FSTAT_QUERIES = 256; // FSTAT_MAX_QUERIES (recompute_fstat.cuh): the recompute search's tile when it may emit

static TopkShape shape_of(bool scan, size_t n, size_t nq, uint32_t k) {
    return scan ? topk_shape_scan(n, nq, k) : topk_shape_recompute(n, nq, k, FSTAT_QUERIES);
}
// the exact scan asks for emission only past its first emission chunk (scan.hip); the recompute search whenever its kernel emits
static bool wanted(bool scan, const TopkShape &s, bool emit) { return emit && (!scan || s.n > s.emit_first); }

static int print_plans() {
    char line[256], who[16];
    while (fgets(line, sizeof line, stdin)) {
        unsigned emit, k;
        unsigned long long n, nq;
        if (sscanf(line, "%15s %u %llu %llu %u", who, &emit, &n, &nq, &k) != 5 || (strcmp(who, "scan") && strcmp(who, "recompute"))) {
            fprintf(stderr, "topk_plan_selftest: bad case line: %s", line);
            return 2;
        }
        const bool scan = strcmp(who, "scan") == 0;
        const TopkShape s = shape_of(scan, n, nq, k);
        const TopkPlan p = topk_plan(s, wanted(scan, s, emit != 0));
        printf("{\"emit\": %d, \"chunks\": [", p.emit ? 1 : 0);
        for (size_t c = 0; c < p.chunks.size(); c++) printf("%s[%zu, %zu]", c ? ", " : "", p.chunks[c].first, p.chunks[c].second);
        printf("], \"slab_rows\": %zu, \"total_segs\": %zu, \"cand_len\": %zu, \"emit_cap\": %u, \"slots\": %zu, \"cnt_off\": %zu, "
               "\"overflow_off\": %zu, \"list_off\": %zu, \"emit_bytes\": %zu}\n",
               p.slab_rows, p.total_segs, p.cand_len, p.emit_cap, p.slots, p.cnt_off, p.overflow_off, p.list_off, p.emit_bytes);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1) return strcmp(argv[1], "--plans") == 0 ? print_plans() : 2;
    const size_t ns[] = {0, 1, 2047, 2048, 2049, 16383, 16384, 16385, 65535, 65536, 65537, 131072, 131073, 524288, 524289, 1000000, 10000000,
                         4294967295ull};
    const size_t nqs[] = {1, 63, 64, 65, 256, 257, 4096, 16384};
    const uint32_t ks[] = {1, 10, 256, 257, 1024};
    long cases = 0, emitting = 0, bad_cover = 0, bad_cap = 0, bad_slab = 0, bad_segs = 0, bad_cand = 0, bad_emit = 0, bad_schedule = 0, bad_block = 0,
         bad_emit_cap = 0;
    for (int scan = 0; scan < 2; scan++)
        for (int want = 0; want < 2; want++)
            for (size_t n : ns)
                for (size_t nq : nqs)
                    for (uint32_t k : ks) {
                        const TopkShape s = shape_of(scan != 0, n, nq, k);
                        const TopkPlan p = topk_plan(s, wanted(scan != 0, s, want != 0));
                        cases++;
                        emitting += p.emit;
                        // chunks: non-empty, contiguous from 0, n rows in all
                        size_t pos = 0;
                        bool cover = true;
                        for (const auto &c : p.chunks) { cover = cover && c.first == pos && c.second > 0; pos += c.second; }
                        if (!cover || pos != n || (n == 0) != p.chunks.empty()) bad_cover++;
                        // slab chunks: within the cap; the slab of the scan (all queries in one pass) within 2^29 scores
                        size_t segs = 0, widest = SEG;
                        for (size_t c = 0; c < p.chunks.size(); c++) {
                            if (p.slab_chunk(c) != (!p.emit || c == 0)) bad_emit++;
                            if (!p.slab_chunk(c)) continue;
                            if (p.chunks[c].second > s.slab_cap) bad_cap++;
                            segs += (p.chunks[c].second + 2047) / 2048;
                            if (p.chunks[c].second > widest) widest = p.chunks[c].second;
                        }
                        if (p.slab_rows != widest || (scan && nq * p.slab_rows > ((size_t)1 << 29))) bad_slab++;
                        if (p.total_segs != (segs ? segs : 1)) bad_segs++;
                        if (p.cand_len != (p.total_segs * k > k ? p.total_segs * k : k)) bad_cand++;
                        if (n == 0 && (p.total_segs != 1 || p.cand_len != k)) bad_segs++;
                        // emission: only when wanted, only with something to emit; then chunk 0 alone goes through the slab
                        if (p.emit && (!want || p.chunks.size() < 2 || p.chunks.size() > 3)) bad_emit++;
                        if (!p.emit && want && (scan ? n > s.emit_first : n > (s.emit_first < s.slab_cap ? s.emit_first : s.slab_cap))) bad_emit++;
                        // the schedules themselves
                        for (size_t c = 0; c < p.chunks.size(); c++) {
                            const size_t left = n - p.chunks[c].first;
                            size_t len;
                            if (p.emit) len = c == 0 ? (s.emit_first < s.slab_cap ? s.emit_first : s.slab_cap) : c == 1 ? s.emit_second : left;
                            else {
                                len = (size_t)128 << 10;
                                for (size_t i = 0; i < c && len < s.slab_cap; i++) len *= 4;
                                if (len > s.slab_cap) len = s.slab_cap;
                            }
                            if (p.chunks[c].second != (len < left ? len : left)) bad_schedule++;
                        }
                        // the emission block: thr | cnt | overflow | list, in this order, no overlap, aligned, `slots` entries each
                        const size_t slots = scan ? (nq + 63) / 64 * 64 : FSTAT_QUERIES;
                        if (p.slots != slots || slots < (scan ? nq : FSTAT_QUERIES) || p.cnt_off < 4 * slots || p.cnt_off % 4 ||
                            p.overflow_off < p.cnt_off + 4 * slots || p.overflow_off % 4 || p.list_off < p.overflow_off + 4 || p.list_off % 8 ||
                            p.emit_bytes != p.list_off + 8 * slots * (size_t)p.emit_cap)
                            bad_block++;
                        if (p.emit_cap != (32 * k > 8192 ? 32 * k : 8192)) bad_emit_cap++;
                    }
    const long bad = bad_cover + bad_cap + bad_slab + bad_segs + bad_cand + bad_emit + bad_schedule + bad_block + bad_emit_cap;
    printf("{\"cases\": %ld, \"emitting\": %ld, \"bad_cover\": %ld, \"bad_cap\": %ld, \"bad_slab\": %ld, \"bad_segs\": %ld, \"bad_cand\": %ld, "
           "\"bad_emit\": %ld, \"bad_schedule\": %ld, \"bad_block\": %ld, \"bad_emit_cap\": %ld}\n",
           cases, emitting, bad_cover, bad_cap, bad_slab, bad_segs, bad_cand, bad_emit, bad_schedule, bad_block, bad_emit_cap);
    return bad ? 1 : 0;
}
