// encode_plan_selftest — the column-block plan of the general recompute encode kernel (csrc/encode_plan.h) on the CPU: no GPU, no
// library.  For every dims in 1..4096 and a set of feature widths it checks that the padded width is a multiple of 128 and covers
// dims, that the blocks tile [0, dp) exactly, that every block width is one the kernels are compiled for, that dims <= 768 keeps the
// one-block plan of encode_kernel<ct, ..> (5 tiles rounded up to 6), and that the LDS figure is that of the widest block and within
// 160 KiB whenever the plan is accepted.  Prints one JSON line; exit status 1 on any violation.
#include "../csrc/encode_plan.h"
#include <cstdio>
#include <vector>

int main() {
    const size_t hs[] = {64, 100, 128, 256, 512, 1024};
    long cases = 0, accepted = 0, bad_dp = 0, bad_tiling = 0, bad_width = 0, bad_narrow = 0, bad_lds = 0, bad_padding = 0, bad_limit = 0;
    int max_blocks = 0;
    for (size_t h : hs) {
        const size_t hp = (h + 15) / 16 * 16;
        for (size_t dims = 1; dims <= LEANN_ENCODE_MAX_DIMS; dims++) {
            const EncodePlan p = encode_plan(h, dims);
            cases++;
            if (!p.ok) { // rejected: no compiled width may fit
                if (encode_lds_bytes(hp, 128, true) <= LEANN_ENCODE_LDS_LIMIT && dims > 768) bad_lds++;
                if (dims <= 768) {
                    const size_t ct = (dims + 127) / 128 == 5 ? 6 : (dims + 127) / 128;
                    if (encode_lds_bytes(hp, ct * 128, true) <= LEANN_ENCODE_LDS_LIMIT) bad_narrow++;
                }
                continue;
            }
            accepted++;
            if (p.dp < dims || p.dp % 128 != 0) bad_dp++;
            if (p.nblk < 1 || p.nblk > LEANN_ENCODE_MAX_BLOCKS) { bad_tiling++; continue; }
            // the blocks, laid end to end in column order, cover every 128-column tile of [0, dp) exactly once
            std::vector<int> cover(p.dp / 128, 0);
            size_t col0 = 0;
            int widest = 0;
            bool overflow = false;
            for (int b = 0; b < p.nblk; b++) {
                if (!encode_ct_compiled(p.ctb[b])) bad_width++;
                for (int t = 0; t < p.ctb[b]; t++) {
                    const size_t tile = col0 / 128 + t;
                    if (tile >= cover.size()) overflow = true;
                    else cover[tile]++;
                }
                col0 += (size_t)p.ctb[b] * 128;
                if (p.ctb[b] > widest) widest = p.ctb[b];
            }
            bool exact = !overflow && col0 == p.dp;
            for (int c : cover) exact = exact && c == 1;
            if (!exact) bad_tiling++;
            if (widest != p.ctb_max) bad_lds++;
            if (p.lds_bytes != encode_lds_bytes(hp, (size_t)widest * 128, true)) bad_lds++;
            if (p.lds_bytes > LEANN_ENCODE_LDS_LIMIT) bad_limit++;
            if (dims <= 768) { // today's plan: one block, ct = ceil(dims / 128) with 5 -> 6
                int ct = (int)((dims + 127) / 128);
                if (ct == 5) ct = 6;
                if (p.nblk != 1 || p.ctb[0] != ct || p.dp != (size_t)ct * 128) bad_narrow++;
            } else {
                if (p.dp != (dims + 127) / 128 * 128) bad_padding++; // no padded tile
                // fewest blocks: an independent count over the widths that fit the LDS budget at this feature width
                int cmax = 0;
                for (int w : {1, 2, 3, 4, 6})
                    if (encode_lds_bytes(hp, (size_t)w * 128, true) <= LEANN_ENCODE_LDS_LIMIT) cmax = w;
                const int tiles = (int)(p.dp / 128);
                std::vector<int> best(tiles + 1, 1 << 20);
                best[0] = 0;
                for (int t = 1; t <= tiles; t++)
                    for (int w : {1, 2, 3, 4, 6})
                        if (w <= cmax && w <= t && best[t - w] + 1 < best[t]) best[t] = best[t - w] + 1;
                if (p.nblk != best[tiles]) bad_tiling++;
                if (p.nblk < 2) bad_tiling++;
            }
            if (p.nblk > max_blocks) max_blocks = p.nblk;
        }
        // past the limit: never a plan
        if (encode_plan(h, LEANN_ENCODE_MAX_DIMS + 1).ok) bad_limit++;
    }
    if (encode_plan(0, 128).ok || encode_plan(256, 0).ok) bad_limit++;
    const long bad = bad_dp + bad_tiling + bad_width + bad_narrow + bad_lds + bad_padding + bad_limit;
    printf("{\"cases\": %ld, \"accepted\": %ld, \"max_blocks\": %d, \"bad_dp\": %ld, \"bad_tiling\": %ld, \"bad_width\": %ld, "
           "\"bad_narrow\": %ld, \"bad_lds\": %ld, \"bad_padding\": %ld, \"bad_limit\": %ld}\n",
           cases, accepted, max_blocks, bad_dp, bad_tiling, bad_width, bad_narrow, bad_lds, bad_padding, bad_limit);
    return bad ? 1 : 0;
}
