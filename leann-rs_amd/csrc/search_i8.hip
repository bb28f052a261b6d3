// search_i8.hip — the beam search over int8 rows (LEANN_ROWS_I8; the row store: rows_i8.hip).  The hop loop is search.cuh's
// beam_search_one, instantiated with I8 = true: only the query staging (q'_j = q_j 2^-e_j, once per query), the row load and the
// conversion differ (wave_dist_rows_i8), so the walk, the visited set, the merge and the filtered result list are the code the f32
// kernels run, and every answer is bit for bit the f32 kernels' answer on the dequantised rows.  A translation unit of its own:
// the kernels of api.hip and search_bf16.hip and their compile times stay as they are.
//
// Scales on the query, not on the row: a row element then costs one conversion (v_cvt_f32_i32 with a sign-extending SDWA byte
// select, no shift or mask) and one fmaf, and the d scales are read once per query instead of once per row.  Dequantising in
// registers costs a multiplication per element and the scales in registers next to the query (T more float4 per lane).
//
// Forms: 16 waves per query for small batches (<= 512 queries, the bf16 threshold: int8 batches were not swept on their own), else
// 4; plain and filtered; lists of <= 64 ids and wide lists (LW = 2).  Row widths: the chunk counts T of the f32 kernels.
//
// Rows in flight per wave (R) and wave counts were read off hipcc's -Rpass-analysis=kernel-resource-usage report over a grid of
// candidates (profiles/i8_rows_resources.md).  An int8 row is one register per chunk where a bf16 row is two.
//   * 4 waves per query: over R in {1, 1.5, 2} x the bf16 kernel's R, the R at which R x min(waves per SIMD the registers allow, 4)
//     — the rows a CU has in flight; the 32 KiB visited table allows 4 workgroups — is largest for the narrow plain and filtered kernel
//     alike (the smaller of the two counts; a tie takes the smaller R): 16, 12, 12, 12, 8, 6, 4, 4 for T = 1, 2, 3, 4, 6, 8, 12, 16.
//   * 16 waves per query: 1 024 work items cap a wave at 128 registers, and a hop's <= 64 unseen rows are at most 4 per wave: R = 4
//     up to T = 6, 3 at T = 8, 1 at T = 12 — the largest that spills no vector register.  At T = 16 R = 1 spills 4 to 8 registers:
//     small batches of rows wider than 3 072 floats run the 4-wave kernel, as they do on bf16 rows.
// No kernel here spills a vector register or contains a scratch instruction.  Throughput was not part of the choice.
#include "common.cuh"
#include "search.cuh"
#include "internal.h"

template <int T, int R, int NW>
__global__ void __launch_bounds__(NW * 64) i8_beam_search_kernel(GraphView g, SearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t qi = blockIdx.x;
    if (qi >= a.nq) return;
    beam_search_one<T, R, NW, false, false, false, 1, false, false, true>(g, a, qi, smem);
}
template <int T, int R, int NW>
__global__ void __launch_bounds__(NW * 64) i8_beam_search_filtered_kernel(GraphView g, SearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t qi = blockIdx.x;
    if (qi >= a.nq) return;
    beam_search_one<T, R, NW, false, true, false, 1, false, false, true>(g, a, qi, smem);
}
template <int T, int R, int NW>
__global__ void __launch_bounds__(NW * 64) wide_i8_beam_search_kernel(GraphView g, SearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t qi = blockIdx.x;
    if (qi >= a.nq) return;
    beam_search_one<T, R, NW, false, false, false, 2, false, false, true>(g, a, qi, smem);
}
template <int T, int R, int NW>
__global__ void __launch_bounds__(NW * 64) wide_i8_beam_search_filtered_kernel(GraphView g, SearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t qi = blockIdx.x;
    if (qi >= a.nq) return;
    beam_search_one<T, R, NW, false, true, false, 2, false, false, true>(g, a, qi, smem);
}

// The table: one row per kernel, the key and the instantiation written from the same template arguments; R by T and by wave count:
// search_plan.h (search_i8_R4 / _R16; R16 = 0: no 16-wave form at this width).
template <int T, int R, int NW, bool WIDE, bool FILT>
static constexpr SearchKernelRow i8_row() {
    SearchKernel k = nullptr;
    if constexpr (WIDE) k = FILT ? wide_i8_beam_search_filtered_kernel<T, R, NW> : wide_i8_beam_search_kernel<T, R, NW>;
    else k = FILT ? i8_beam_search_filtered_kernel<T, R, NW> : i8_beam_search_kernel<T, R, NW>;
    return {SEARCH_I8, T, R, NW, WIDE, FILT, false, k};
}
#define I8_FORMS(T, R, NW) i8_row<T, R, NW, false, false>(), i8_row<T, R, NW, false, true>(), i8_row<T, R, NW, true, false>(), i8_row<T, R, NW, true, true>()
#define I8_WIDTH(T) I8_FORMS(T, search_i8_R4(T), 4), I8_FORMS(T, search_i8_R16(T), 16)

// the kernel of a plan of the I8 family (search_plan.h); leann_internal_launch_search launches it as it does every other
int leann_internal_i8_kernel(const GraphView &g, const SearchPlan &p, SearchKernel *out) {
    if (!g.X || !g.norms || g.feat_h || (g.row_bytes & 127u) || g.row_bytes < g.ld) {
        leann_set_error("int8 rows: the handle's row store or its column scales are missing or malformed (pitch %u B for %u elements)", g.row_bytes,
                        g.ld);
        return LEANN_ERR_INVALID;
    }
    static constexpr SearchKernelRow rows[] = {
        I8_WIDTH(1), I8_WIDTH(2), I8_WIDTH(3), I8_WIDTH(4), I8_WIDTH(6), I8_WIDTH(8), I8_WIDTH(12), I8_FORMS(16, search_i8_R4(16), 4),
    };
    return leann_internal_find_kernel(rows, p, out);
}
