/* selfcheck.c — small driver exercising every oracle entry point; built with
 * -fsanitize=address,undefined by `make -C oracle selfcheck` (sanitizers run on the CPU build only). */
#include "oracle.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
int main(void) {
    const uint32_t d = 48, n = 1500, nq = 40;
    float *X = malloc((size_t)n * d * 4), *Q = malloc((size_t)nq * d * 4);
    orc_gen_rows(7, d, 16, 32, 1.0f, 0, 0, n, X);
    orc_gen_rows(7, d, 16, 32, 1.0f, 1, 0, nq, Q);
    orc_graph *g = orc_hnsw_build(X, n, d, 8, 32, 3);
    uint64_t keys[2][40 * 10]; float dist[2][40 * 10]; uint32_t cnt[2][40]; uint64_t st[40 * 3];
    orc_graph_search_batch(g, Q, nq, 10, 50, 0, 4, keys[0], dist[0], cnt[0], st);
    orc_graph_search_batch(g, Q, nq, 10, 50, 1, 2, keys[1], dist[1], cnt[1], NULL);
    if (memcmp(keys[0], keys[1], sizeof keys[0]) || memcmp(dist[0], dist[1], sizeof dist[0])) { puts("FAIL: algo 0 != algo 1"); return 1; }
    uint64_t info[8]; orc_graph_info(g, info);
    uint8_t *lv = malloc(n); uint32_t *uo = malloc(n * 4), *a0 = malloc((size_t)n * info[4] * 4), *aU = malloc((info[7] + 1) * info[3] * 4);
    orc_graph_export(g, lv, uo, a0, aU);
    orc_graph *g2 = orc_graph_from_arrays(X, n, d, d, (uint32_t)info[3], (uint32_t)info[4], (uint32_t)info[5], (uint32_t)info[6], lv, uo, a0, aU, info[7]);
    uint64_t k2[10]; float d2[10]; uint32_t c2; uint64_t s2[3];
    orc_graph_search(g2, Q, 10, 50, 0, k2, d2, &c2, s2);
    if (memcmp(k2, keys[0], sizeof k2)) { puts("FAIL: export/import"); return 1; }
    orc_graph *v = orc_vamana_build(X, 600, d, 12, 24, 1.2f, 5);
    orc_graph_search(v, Q, 10, 30, 1, k2, d2, &c2, s2);
    {
        uint64_t lk[50], le[8], bk[3 * 50], be[3 * 8]; uint32_t ln, lne, bc[3], bn[3], rows[3] = {1, 700, 1499}, pos[10], pid[10]; float pd[10];
        orc_graph_search_level(g, Q, 0, 50, 0, lk, &ln, le, 8, &lne);
        orc_graph_search(g, Q, 50, 50, 0, keys[1], dist[1], &c2, NULL);
        if (ln != c2 || lne == 0) { puts("FAIL: level search count"); return 1; }
        for (uint32_t i = 0; i < ln; i++)
            if ((uint32_t)lk[i] != (uint32_t)keys[1][i]) { puts("FAIL: level search != search at level 0"); return 1; }
        orc_graph_search_level(g, Q, 99, 50, 0, lk, &ln, le, 8, &lne);
        if (ln || lne) { puts("FAIL: level above max_level"); return 1; }
        orc_graph_search_level_batch(g, rows, 3, 1, 50, 0, 2, bk, bc, be, 8, bn);
        orc_graph_search_level_batch(v, rows, 2, 0, 50, 1, 1, bk, bc, NULL, 0, NULL);
        for (uint32_t i = 0; i < 10; i++) { pid[i] = (uint32_t)bk[i]; pd[i] = orc_orderable_f32((uint32_t)(bk[i] >> 32)); }
        if (orc_prune(X, d, d, pid, pd, 10, 4, 1.2f, 1, pos) < 1 || orc_prune(X, d, d, pid, pd, 10, 4, 0.0f, 0, pos) < 1) { puts("FAIL: prune"); return 1; }
    }
    {   /* the counting search: same answers as the plain one, something ruled out, the bound below the distance */
        uint64_t ck[40 * 10], cst[40 * 3], ruled[40], r1, total = 0; float cd[40 * 10]; uint32_t cc[40];
        for (int algo = 0; algo < 2; algo++) {
            if (orc_graph_search_counted_batch(g, Q, nq, 10, 50, algo, 3, ck, cd, cc, cst, ruled)) { puts("FAIL: counted batch"); return 1; }
            if (memcmp(ck, keys[0], sizeof ck) || memcmp(cd, dist[0], sizeof cd) || memcmp(cc, cnt[0], sizeof cc)) { puts("FAIL: counted != plain"); return 1; }
            if (algo == 0 && memcmp(cst, st, sizeof cst)) { puts("FAIL: counted stats"); return 1; }
            for (uint32_t i = 0; i < nq; i++) { total += ruled[i]; if (ruled[i] >= cst[3 * i]) { puts("FAIL: more ruled out than evaluated"); return 1; } }
            if (orc_graph_search_counted(g, Q, 10, 50, algo, k2, d2, &c2, s2, &r1) || r1 != ruled[0]) { puts("FAIL: counted single"); return 1; }
        }
        if (!total) { puts("FAIL: nothing ruled out"); return 1; }
        orc_graph_search_counted(v, Q, 1, 1, 1, k2, d2, &c2, s2, &r1);
        for (uint32_t i = 0; i < 200; i++)
            if (!(orc_screen_lb(Q, X + (size_t)i * d, d) <= orc_dist_canon(Q, X + (size_t)i * d, d))) { puts("FAIL: lb > dist"); return 1; }
        float one = 1.0f;
        if (!(orc_screen_lb(&one, &one, 1) <= 0.0f)) { puts("FAIL: lb, d = 1"); return 1; }
    }
    uint64_t sk[5]; float ss[5]; uint32_t sn; uint8_t mask[(1500 + 7) / 8]; memset(mask, 0x55, sizeof mask);
    orc_scan_topk(X, n, d, Q, 5, 0, mask, sk, ss, &sn);
    uint64_t mk[10]; float md[10]; uint32_t mn;
    orc_merge_topk(keys[0], dist[0], cnt[0], 4, 10, 10, mk, md, &mn);
    uint64_t hi[3] = {0, 1, 2}, ho[3]; float hv[3] = {0.9f, 0.8f, 0.7f}, hb[3] = {0.5f, 0.9f, 0.3f}, hs[3];
    orc_hybrid_rerank(hi, hv, 3, hb, 3, 0.5f, ho, hs);
    uint16_t *F = malloc(100 * 32 * 2), *W = malloc(32 * d * 2); float *E = malloc(100 * d * 4);
    orc_synth_features(1, 32, 8, 8, 1.0f, 0, 0, 100, F); orc_synth_weights(1, 32, d, W); orc_recompute_encode(F, 100, 32, W, d, E);
    orc_graph_free(g); orc_graph_free(g2); orc_graph_free(v);
    free(X); free(Q); free(lv); free(uo); free(a0); free(aU); free(F); free(W); free(E);
    puts("oracle selfcheck OK");
    return 0;
}
