// row_screen_selftest.cpp — CPU check of the row screen's bound (csrc/row_screen.h): over random and adversarial rows the lower bound
// the screen computes from the upper 16 bits of a row must never exceed the canonical distance computed from the whole row.  Both
// chains are restated here in the device code's order (lane l owns elements 256 t + 4 l .. + 3; 4 fmaf chains, two in-lane additions,
// the adjacent-pair tree over 64 lanes), in f32 with fmaf, compiled without contraction.  No GPU.  Prints one JSON object.
// With a file argument: the file holds cases, each a u32 d (1 .. 4096) followed by d f32 of a query and d f32 of a row; per case one
// line "<bits of screen_lb> <bits of canon_dist>" in hex, T = ceil(d / 256), from the same two functions — what the device compiles
// of row_screen.h — so that a second statement of the bound (oracle/oracle.c: orc_screen_lb) can be held to this one bit for bit
// (tests/test_cpu_row_screen.py).
#include "../csrc/row_screen.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { // splitmix64
    uint64_t x = (rng_state += 0x9E3779B97F4A7C15ull);
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
static float uni() { return (float)((rnd() >> 40) + 1) * (1.0f / 16777217.0f); }
static float gauss() { return sqrtf(-2.0f * logf(uni())) * cosf(6.2831853f * uni()); }

static float tree64(float *v) {
    for (int w = 32; w >= 1; w >>= 1)
        for (int i = 0; i < w; i++) v[i] = v[2 * i] + v[2 * i + 1];
    return v[0];
}
// canonical distance of the whole row (common.cuh: fma4 / lane4_sum / wave_tree_sum); d <= 256 T, operands zero padded
static float canon_dist(const float *q, const float *x, int T) {
    float lane[64];
    for (int l = 0; l < 64; l++) {
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        for (int t = 0; t < T; t++)
            for (int e = 0; e < 4; e++) a[e] = fmaf(q[256 * t + 4 * l + e], x[256 * t + 4 * l + e], a[e]);
        lane[l] = (a[0] + a[1]) + (a[2] + a[3]);
    }
    return 1.0f - tree64(lane);
}
// the screen (search.cuh: wave_dist_rows_screen) on the upper halves alone
static float screen_lb(const float *q, const float *x, int T) {
    float lane[64], qs[64];
    for (int l = 0; l < 64; l++) {
        float s[4] = {0.f, 0.f, 0.f, 0.f}, a[4] = {0.f, 0.f, 0.f, 0.f}, qa[4] = {0.f, 0.f, 0.f, 0.f};
        for (int t = 0; t < T; t++)
            for (int e = 0; e < 4; e++) {
                const float qe = q[256 * t + 4 * l + e], hi = rs_join(rs_hi16(x[256 * t + 4 * l + e]), 0);
                s[e] = fmaf(qe, hi, s[e]);
                a[e] = fmaf(fabsf(qe), fabsf(hi), a[e]);
                qa[e] += fabsf(qe);
            }
        lane[l] = rs_lane_bound((s[0] + s[1]) + (s[2] + s[3]), (a[0] + a[1]) + (a[2] + a[3]));
        qs[l] = (qa[0] + qa[1]) + (qa[2] + qa[3]);
    }
    return rs_lower_bound(tree64(lane), rs_abs_term(tree64(qs)));
}

static void normalize(std::vector<float> &v, int d, float scale) {
    double n = 0;
    for (int i = 0; i < d; i++) n += (double)v[i] * v[i];
    n = n > 0 ? scale / sqrt(n) : 0;
    for (int i = 0; i < d; i++) v[i] = (float)(v[i] * n);
}

static int print_cases(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "row_screen_selftest: cannot open %s\n", path); return 2; }
    uint32_t d;
    while (fread(&d, 4, 1, f) == 1) {
        if (d < 1 || d > 4096) { fprintf(stderr, "row_screen_selftest: d = %u\n", d); fclose(f); return 2; }
        const int T = ((int)d + 255) / 256;
        std::vector<float> q(256 * T, 0.f), x(256 * T, 0.f);
        if (fread(q.data(), 4, d, f) != d || fread(x.data(), 4, d, f) != d) { fprintf(stderr, "row_screen_selftest: short case\n"); fclose(f); return 2; }
        printf("%08x %08x\n", rs_f32_to_bits(screen_lb(q.data(), x.data(), T)), rs_f32_to_bits(canon_dist(q.data(), x.data(), T)));
    }
    fclose(f);
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1) return print_cases(argv[1]);
    unsigned long long cases = 0, violations = 0, roundtrip_bad = 0, layout_bad = 0;
    double max_gap = 0, min_gap = 1e30; // canonical distance - lower bound (must be >= 0; how sharp the bound is)
    const int dims[] = {768, 1536, 700, 1, 37, 256, 4096};
    const float scales[] = {1.0f, 1e-3f, 37.5f, 1e-20f, 1e15f};
    for (int d : dims) {
        const int T = (d + 255) / 256;
        std::vector<float> q(256 * T, 0.f), x(256 * T, 0.f), c(256 * T, 0.f);
        for (int rep = 0; rep < (d > 2000 ? 40 : 150); rep++) {
            const float sq = scales[rnd() % 5], sx = scales[rnd() % 5];
            for (int i = 0; i < d; i++) { q[i] = gauss(); c[i] = gauss(); }
            normalize(q, d, sq);
            for (int mode = 0; mode < 6; mode++) {
                // 0 random row; 1 near-duplicate of the query; 2 near the query, low halves forced to the worst case of the truncation
                // (0xFFFF where sign(x) == sign(q), 0 elsewhere); 3 the opposite forcing; 4 as 2 with zero / subnormal / tiny elements
                // sprinkled in; 5 anti-correlated with forcing
                for (int i = 0; i < d; i++) x[i] = mode == 0 ? c[i] : (mode == 5 ? -1.f : 1.f) * q[i] / (sq > 0 ? sq : 1.f) + 1e-3f * c[i];
                normalize(x, d, sx);
                if (mode >= 2)
                    for (int i = 0; i < d; i++) {
                        uint32_t b = rs_f32_to_bits(x[i]);
                        const bool same = ((b >> 31) != 0) == (q[i] < 0.f);
                        b = (b & 0xFFFF0000u) | ((same != (mode == 3)) ? 0xFFFFu : 0u);
                        x[i] = rs_bits_to_f32(b);
                    }
                if (mode == 4)
                    for (int i = 0; i < d; i += 7) {
                        const uint32_t sign = (uint32_t)(rnd() & 1) << 31;
                        const uint32_t pick = (uint32_t)(rnd() % 4);
                        x[i] = rs_bits_to_f32(sign | (pick == 0 ? 0u : pick == 1 ? 0x0000FFFFu : pick == 2 ? 0x007FFFFFu : 0x00800000u | 0xFFFFu));
                    }
                const float dist = canon_dist(q.data(), x.data(), T), lb = screen_lb(q.data(), x.data(), T);
                cases++;
                if (!(lb <= dist)) violations++;
                const double gap = (double)dist - (double)lb;
                if (gap > max_gap) max_gap = gap;
                if (gap < min_gap) min_gap = gap;
                for (int i = 0; i < d; i++)
                    if (rs_f32_to_bits(rs_join(rs_hi16(x[i]), rs_lo16(x[i]))) != rs_f32_to_bits(x[i])) roundtrip_bad++;
            }
        }
    }
    // the plane layout is a permutation of each row, groups of four stay together and 8-byte aligned
    for (uint32_t ldp = 64; ldp <= 4096; ldp += 64) {
        std::vector<int> seen(ldp, 0);
        for (uint32_t j = 0; j < ldp; j++) {
            const uint32_t p = rs_plane_pos(j, ldp);
            if (p >= ldp || seen[p]++) layout_bad++;
            if ((j & 3u) == 0 && (p & 3u)) layout_bad++;
            if ((j & 3u) && p != rs_plane_pos(j & ~3u, ldp) + (j & 3u)) layout_bad++;
        }
    }
    printf("{\"cases\": %llu, \"violations\": %llu, \"roundtrip_bad\": %llu, \"layout_bad\": %llu, \"min_gap\": %.9g, \"max_gap\": %.9g}\n", cases,
           violations, roundtrip_bad, layout_bad, min_gap, max_gap);
    return violations || roundtrip_bad || layout_bad ? 1 : 0;
}
