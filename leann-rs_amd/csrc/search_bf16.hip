// search_bf16.hip — the beam search over bf16 rows (LEANN_ROWS_BF16; the row store: rows_bf16.hip).  The hop loop is search.cuh's
// beam_search_one, instantiated with BF16 = true: only the row load and the widening differ (wave_dist_rows_bf16), so the walk, the
// visited set, the merge and the filtered result list are the code the f32 kernels run, and every answer is bit for bit the f32
// kernels' answer on the widened rows.  A translation unit of its own: api.hip's kernels and its compile time stay as they are.
//
// Forms: 16 waves per query for small batches (<= 512 queries, as the recompute-on launcher), else 4; plain and filtered; lists of
// <= 64 ids and wide lists (LW = 2).  Row widths: the chunk counts T of the f32 kernels, T = ceil(ld / 256) mapped the same
// way (search_plan.h: 5 -> 6, 7 -> 8, 9..11 -> 12, 13..15 -> 16; the extra chunks read as zeros and add +0 products, as they do there).
//
// Rows in flight per wave (R) and wave counts were read off hipcc's -Rpass-analysis=kernel-resource-usage report over a grid of
// candidates (profiles/bf16_rows_resources.md), not guessed.  A bf16 row is two registers per chunk where an f32 row is four.
//   * 4 waves per query (throughput): the largest R <= twice the f32 kernel's whose narrow plain and filtered kernels spill nothing
//     and keep R x (workgroups per CU the registers allow) — the rows a CU has in flight — at its maximum: 8, 8, 8, 6, 4, 4, 2, 2 for
//     T = 1, 2, 3, 4, 6, 8, 12, 16.  Up to T = 6 that is 4 workgroups per CU, what the 32 KiB visited table allows anyway.
//   * 16 waves per query (small batches): 1 024 work items cap a wave at 128 registers, and a hop's <= 64 (wide: 128) unseen rows
//     are at most 4 (8) per wave: R = 4 up to T = 4, then 3, 2, 1 — the largest that does not spill.  At T = 16 the query alone is 64
//     registers and no R fits (R = 1 spills 14 to 21 registers): small batches of rows wider than 3 072 floats run the 4-wave kernel.
// No kernel here spills a vector register or contains a scratch instruction.
#include "common.cuh"
#include "search.cuh"
#include "internal.h"

template <int T, int R, int NW>
__global__ void __launch_bounds__(NW * 64) bf16_beam_search_kernel(GraphView g, SearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t qi = blockIdx.x;
    if (qi >= a.nq) return;
    beam_search_one<T, R, NW, false, false, false, 1, false, true>(g, a, qi, smem);
}
template <int T, int R, int NW>
__global__ void __launch_bounds__(NW * 64) bf16_beam_search_filtered_kernel(GraphView g, SearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t qi = blockIdx.x;
    if (qi >= a.nq) return;
    beam_search_one<T, R, NW, false, true, false, 1, false, true>(g, a, qi, smem);
}
template <int T, int R, int NW>
__global__ void __launch_bounds__(NW * 64) wide_bf16_beam_search_kernel(GraphView g, SearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t qi = blockIdx.x;
    if (qi >= a.nq) return;
    beam_search_one<T, R, NW, false, false, false, 2, false, true>(g, a, qi, smem);
}
template <int T, int R, int NW>
__global__ void __launch_bounds__(NW * 64) wide_bf16_beam_search_filtered_kernel(GraphView g, SearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t qi = blockIdx.x;
    if (qi >= a.nq) return;
    beam_search_one<T, R, NW, false, true, false, 2, false, true>(g, a, qi, smem);
}

// The table: one row per kernel, the key and the instantiation written from the same template arguments; R by T and by wave count:
// search_plan.h (search_bf16_R4 / _R16; R16 = 0: no 16-wave form at this width).
template <int T, int R, int NW, bool WIDE, bool FILT>
static constexpr SearchKernelRow bf16_row() {
    SearchKernel k = nullptr;
    if constexpr (WIDE) k = FILT ? wide_bf16_beam_search_filtered_kernel<T, R, NW> : wide_bf16_beam_search_kernel<T, R, NW>;
    else k = FILT ? bf16_beam_search_filtered_kernel<T, R, NW> : bf16_beam_search_kernel<T, R, NW>;
    return {SEARCH_BF16, T, R, NW, WIDE, FILT, false, k};
}
#define BF16_FORMS(T, R, NW) bf16_row<T, R, NW, false, false>(), bf16_row<T, R, NW, false, true>(), bf16_row<T, R, NW, true, false>(), bf16_row<T, R, NW, true, true>()
#define BF16_WIDTH(T) BF16_FORMS(T, search_bf16_R4(T), 4), BF16_FORMS(T, search_bf16_R16(T), 16)

// the kernel of a plan of the BF16 family (search_plan.h); leann_internal_launch_search launches it as it does every other
int leann_internal_bf16_kernel(const GraphView &g, const SearchPlan &p, SearchKernel *out) {
    if (!g.X || g.feat_h || (g.row_bytes & 127u) || (size_t)g.row_bytes < 2 * (size_t)g.ld) {
        leann_set_error("bf16 rows: the handle's row store is missing or malformed (pitch %u B for %u elements)", g.row_bytes, g.ld);
        return LEANN_ERR_INVALID;
    }
    static constexpr SearchKernelRow rows[] = {
        BF16_WIDTH(1), BF16_WIDTH(2), BF16_WIDTH(3), BF16_WIDTH(4), BF16_WIDTH(6), BF16_WIDTH(8), BF16_WIDTH(12), BF16_FORMS(16, search_bf16_R4(16), 4),
    };
    return leann_internal_find_kernel(rows, p, out);
}
