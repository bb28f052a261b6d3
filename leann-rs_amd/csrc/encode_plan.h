// encode_plan.h — how the general encode kernel (recompute.hip: encode_kernel / encode_blocked_kernel) covers the columns of W.
// Plain C++ on purpose: leann_recompute_create and the stand-alone host test (host/encode_plan_selftest.cpp) compile the same functions.
//
// A workgroup keeps a 128-passage x CT*128-column tile in accumulators (CT column tiles of 32 per wave, 4 column groups) and stages
// 3 k-step slabs of the same width in LDS; CT is compiled for 1, 2, 3, 4 and 6, so one tile holds at most 768 columns.
//   dims <= 768: ONE block of ct = ceil(dims / 128) tiles, 5 rounded up to 6 (encode_kernel<ct, ..>, unchanged).
//   dims >  768: the padded width dp = ceil(dims / 128) * 128 (no padded tile: a block of one tile is always available) is cut
//                into the FEWEST blocks of compiled widths that fit the LDS budget, widest first (encode_blocked_kernel).
// dp is a multiple of 128 in both cases (fused_fstat_kernel streams W in sub-slices of 128 columns); columns [dims, dp) of the tiled
// weights are zero and add exactly 0 to every sum.
#pragma once
#include <stddef.h>

#define LEANN_ENCODE_MAX_DIMS 4096   // the stored-vector path's limit (api.hip: "dims > 4096 not supported")
#define LEANN_ENCODE_MAX_BLOCKS 32   // 4096 / 128 blocks of one tile
#define LEANN_ENCODE_LDS_LIMIT (160 * 1024)

struct EncodePlan {
    int ok;            // 0: no block width fits the LDS budget at this feature width
    size_t dp;         // padded columns of the tiled weights
    int nblk;          // column blocks, in column order
    int ctb[LEANN_ENCODE_MAX_BLOCKS]; // tiles of 128 columns per block; sum = dp / 128
    int ctb_max;       // the widest block: it sizes the LDS ring
    size_t lds_bytes;  // encode_lds_bytes(hp, ctb_max * 128, fused = true)
};

// sF[128][hp + 8] bf16 + 3 k-step slabs of (columns + the three 64-query pieces of G when fused) x 16 bf16 + sN / sM / sC
static inline size_t encode_lds_bytes(size_t hp, size_t cols, bool fused = false) {
    return 128 * (hp + 8) * 2 + 3 * (cols + (fused ? 192 : 0)) * 16 * 2 + 6 * 128 * 4;
}
static inline constexpr bool encode_ct_compiled(int ct) { return ct == 1 || ct == 2 || ct == 3 || ct == 4 || ct == 6; }

static inline EncodePlan encode_plan(size_t h, size_t dims) {
    EncodePlan p = {};
    const size_t hp = (h + 15) / 16 * 16;
    if (h == 0 || dims == 0 || dims > LEANN_ENCODE_MAX_DIMS) return p;
    const int tiles = (int)((dims + 127) / 128);
    if (dims <= 768) {
        const int ct = tiles == 5 ? 6 : tiles;
        p.dp = (size_t)ct * 128;
        p.nblk = 1;
        p.ctb[0] = p.ctb_max = ct;
        p.lds_bytes = encode_lds_bytes(hp, p.dp, true);
        p.ok = p.lds_bytes <= LEANN_ENCODE_LDS_LIMIT;
        return p;
    }
    p.dp = (size_t)tiles * 128;
    static const int widths[5] = {6, 4, 3, 2, 1}; // widest first
    int cmax = 0;
    for (int w = 4; w >= 0; w--)
        if (encode_lds_bytes(hp, (size_t)widths[w] * 128, true) <= LEANN_ENCODE_LDS_LIMIT) cmax = widths[w];
    if (cmax == 0) {
        p.lds_bytes = encode_lds_bytes(hp, 128, true);
        return p;
    }
    int best[LEANN_ENCODE_MAX_BLOCKS + 1]; // fewest blocks that tile t tiles exactly
    best[0] = 0;
    for (int t = 1; t <= tiles; t++) {
        best[t] = t; // t blocks of one tile
        for (int w = 0; w < 5; w++)
            if (widths[w] <= cmax && widths[w] <= t && best[t - widths[w]] + 1 < best[t]) best[t] = best[t - widths[w]] + 1;
    }
    for (int t = tiles; t > 0;) {
        for (int w = 0; w < 5; w++)
            if (widths[w] <= cmax && widths[w] <= t && best[t - widths[w]] == best[t] - 1) {
                p.ctb[p.nblk++] = widths[w];
                if (widths[w] > p.ctb_max) p.ctb_max = widths[w];
                t -= widths[w];
                break;
            }
    }
    p.lds_bytes = encode_lds_bytes(hp, (size_t)p.ctb_max * 128, true);
    p.ok = 1;
    return p;
}
