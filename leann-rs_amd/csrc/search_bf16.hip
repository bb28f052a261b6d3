// search_bf16.hip — the beam search over bf16 rows (LEANN_ROWS_BF16; the row store: rows_bf16.hip).  The hop loop is search.cuh's
// beam_search_one, instantiated with BF16 = true: only the row load and the widening differ (wave_dist_rows_bf16), so the walk, the
// visited set, the merge and the filtered result list are the code the f32 kernels run, and every answer is bit for bit the f32
// kernels' answer on the widened rows.  A translation unit of its own: api.hip's kernels and its compile time stay as they are.
//
// Forms: 16 waves per query for small batches (<= 512 queries, as the recompute-on launcher), else 4; plain and filtered; lists of
// <= 64 ids and wide lists (LW = 2).  Row widths: the chunk counts T of api.hip's launch_search_T, T = ceil(ld / 256) mapped the same
// way (5 -> 6, 7 -> 8, 9..11 -> 12, 13..15 -> 16: the extra chunks read as zeros and add +0 products, as they do there).
//
// Rows in flight per wave (R) and wave counts were read off hipcc's -Rpass-analysis=kernel-resource-usage report over a grid of
// candidates (profiles/bf16_rows_resources.md), not guessed.  A bf16 row is two registers per chunk where an f32 row is four.
//   * 4 waves per query (throughput): the largest R <= twice launch_search_T's whose narrow plain and filtered kernels spill nothing
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

using SearchKernel = void (*)(GraphView, SearchArgs);

// R4 / R16: rows in flight per wave of the 4- and the 16-wave form; R16 = 0: no 16-wave form at this width
template <int T, int R4, int R16>
static int launch_bf16_T(const GraphView &g, const SearchArgs &a, hipStream_t st) {
    const bool small = R16 != 0 && a.nq <= 512, wide = std::max(g.M0, g.M) > 64, filt = a.allow != nullptr;
    const size_t lds = search_lds_bytes(a.ef, std::max(g.M0, g.M), a.hash_bits, filt ? a.k : 0u, small ? 2u : 1u);
    if (lds > 160 * 1024) {
        leann_set_error("search: complexity %u needs %zu B of LDS per query (> 160 KiB)", a.ef, lds);
        return LEANN_ERR_INVALID;
    }
    SearchKernel k = wide ? (filt ? wide_bf16_beam_search_filtered_kernel<T, R4, 4> : wide_bf16_beam_search_kernel<T, R4, 4>)
                          : (filt ? bf16_beam_search_filtered_kernel<T, R4, 4> : bf16_beam_search_kernel<T, R4, 4>);
    if constexpr (R16 != 0)
        if (small)
            k = wide ? (filt ? wide_bf16_beam_search_filtered_kernel<T, R16, 16> : wide_bf16_beam_search_kernel<T, R16, 16>)
                     : (filt ? bf16_beam_search_filtered_kernel<T, R16, 16> : bf16_beam_search_kernel<T, R16, 16>);
    if (lds > 64 * 1024)
        HIP_CHECK_RET(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL(k, dim3(a.nq), dim3(small ? 16 * 64 : 4 * 64), lds, st, g, a);
    HIP_CHECK_RET(hipGetLastError());
    return LEANN_OK;
}

// `a` arrives complete from leann_internal_launch_search (beam, visited-table size, pools): what is left is the kernel.
int leann_internal_launch_search_bf16(const GraphView &g, const SearchArgs &a, hipStream_t st) {
    if (a.q_rows) { leann_set_error("bf16 rows: construction searches are not supported"); return LEANN_ERR_UNSUPPORTED; }
    if (!g.X || g.feat_h || (g.row_bytes & 127u) || (size_t)g.row_bytes < 2 * (size_t)g.ld) {
        leann_set_error("bf16 rows: the handle's row store is missing or malformed (pitch %u B for %u elements)", g.row_bytes, g.ld);
        return LEANN_ERR_INVALID;
    }
    switch ((int)((g.ld + 255) / 256)) {
        case 1: return launch_bf16_T<1, 8, 4>(g, a, st);
        case 2: return launch_bf16_T<2, 8, 4>(g, a, st);
        case 3: return launch_bf16_T<3, 8, 4>(g, a, st);
        case 4: return launch_bf16_T<4, 6, 4>(g, a, st);
        case 5: case 6: return launch_bf16_T<6, 4, 3>(g, a, st);
        case 7: case 8: return launch_bf16_T<8, 4, 2>(g, a, st);
        case 9: case 10: case 11: case 12: return launch_bf16_T<12, 2, 1>(g, a, st);
        case 13: case 14: case 15: case 16: return launch_bf16_T<16, 2, 0>(g, a, st);
        default:
            leann_set_error("search: dims %u > 4096 not supported", g.d);
            return LEANN_ERR_INVALID;
    }
}
