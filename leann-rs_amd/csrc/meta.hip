// meta.hip — metadata filters evaluated on the device from a columnar store (include/leann_backend.h "metadata filters
// evaluated on the device").  The reference's IndexSearcher answers a filter by parsing every passage's JSON and calling
// MetadataFilter::matches on it (src/index/filter.rs:319-373); here the passages' fields are columns in HBM — tag u8, number f64,
// string code u32 per row — and one kernel evaluates the compiled filter (meta_plan.h: the reduction of every op to a tag mask, a
// number test and a code test) for all rows into an allow-bitmap, which every filtered search of the library takes as it is.
//
// meta_eval_kernel: a wave takes 64 consecutive rows per step, lane = row, so a column's loads are coalesced (64 B of tags, 256 B of
// codes, 512 B of numbers per wave instruction).  A condition's outcome over the 64 rows is one __ballot; the AND / OR program folds
// those wave-uniform masks on a small stack.  Masks and stack live in LDS (328 B per wave) because the program indexes them by
// instruction: in registers that indexing would go through scratch.  Every lane writes the same value to the same LDS word and reads
// back what it wrote, so no barrier is needed.  Conditions come grouped by column: a column's tag is read once per step, its number /
// code only by the lanes whose tag says NUMBER / STRING and only if some condition tests them.  The answer is ANDed with the row's
// validity and an optional second bitmap, written as 8 single bytes per step (a caller's bitmap need not be aligned, and no byte
// behind ceil(n / 8) is written: rows behind n are never allowed, so pad bits are zero), and counted: popcount per step, one atomic per
// workgroup.  Small: 1 + 8 or 4 bytes per row and column touched, 1/8 byte out.  Measured (profiles/meta_filter.md) it is bound by the
// latency of a step's dependent loads — tag, then number or code — not by bandwidth: 0.09 ms for one column of 10M rows.
// meta_eval_batch_kernel (further down) evaluates a planned batch of filters — one bitmap per query of a batch — in one pass.
#include "common.cuh"
#include "../../include/leann_backend.h"
#include "internal.h"
#include "meta_plan.h"
#include "meta_batch_plan.h"
#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#define META_WAVES 4      // per workgroup
#define META_MAX_GRID 2048

struct MetaColumn {
    std::string field;
    std::vector<std::string> dict; // distinct strings, bytewise ascending: read by the filter compiler only
    DeviceBuf<uint8_t> tag;
    DeviceBuf<double> num;    // empty when no row is a NUMBER
    DeviceBuf<uint32_t> code; // empty when no row is a STRING
};
struct leann_meta {
    int device = 0;
    size_t n = 0;
    DeviceBuf<uint8_t> valid; // empty: every row is valid
    mutable std::mutex mu;    // columns, words
    std::vector<std::unique_ptr<MetaColumn>> cols;
    mutable std::map<hipStream_t, DeviceBuf<uint32_t>> words; // per stream: the number sets and bitsets of the evaluation enqueued last
    mutable std::map<hipStream_t, DeviceBuf<unsigned char>> batch; // per stream: programs, pairs and words of the batch enqueued last
};

struct MetaKernelArgs {
    MetaProgram P;
    const uint8_t *tag[MP_MAX_COLS];
    const double *num[MP_MAX_COLS];
    const uint32_t *code[MP_MAX_COLS];
    const uint32_t *words;
    const uint8_t *valid, *extra; // optional bitmaps ANDed in, in this order
    uint8_t *out;
    uint32_t *count; // optional, zero at launch
    uint64_t n;
};

__global__ void __launch_bounds__(64 * META_WAVES) meta_eval_kernel(const MetaKernelArgs a) {
    __shared__ unsigned long long cmask[META_WAVES][MP_MAX_CONDS];
    __shared__ unsigned long long stack[META_WAVES][MP_MAX_DEPTH + 1];
    __shared__ uint32_t wave_count[META_WAVES];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t n_steps = (a.n + 63) / 64, n_bytes = (a.n + 7) / 8;
    uint32_t allowed = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * META_WAVES + w; g < n_steps; g += (uint64_t)gridDim.x * META_WAVES) {
        const uint64_t row = g * 64 + lane;
        bool ok = row < a.n;
        if (ok && a.valid) ok = (a.valid[row >> 3] >> (row & 7)) & 1;
        if (ok && a.extra) ok = (a.extra[row >> 3] >> (row & 7)) & 1;
        unsigned long long res = __ballot(ok);
        if (res) { // (wave-uniform)
            for (uint32_t s = 0; s < a.P.n_cols; s++) {
                const uint32_t tag = ok ? a.tag[s][row] : (uint32_t)LEANN_META_MISSING;
                double num = 0.0;
                uint32_t code = 0;
                if (tag == LEANN_META_NUMBER && (a.P.col_need[s] & 1)) num = a.num[s][row];
                if (tag == LEANN_META_STRING && (a.P.col_need[s] & 2)) code = a.code[s][row];
                for (uint32_t i = a.P.col_first[s]; i < a.P.col_first[s + 1]; i++)
                    cmask[w][i] = __ballot(meta_cond_test(a.P.cond[i], a.words, tag, num, code));
            }
            res &= meta_run_program<unsigned long long>(a.P, stack[w], [&](uint32_t i) { return cmask[w][i]; });
        }
        const uint64_t byte = g * 8 + lane;
        if (lane < 8 && byte < n_bytes) a.out[byte] = (uint8_t)(res >> (8 * lane));
        allowed += (uint32_t)__popcll(res);
    }
    if (lane == 0) wave_count[w] = allowed;
    __syncthreads();
    if (threadIdx.x == 0 && a.count) {
        uint32_t sum = 0;
        for (int i = 0; i < META_WAVES; i++) sum += wave_count[i];
        if (sum) atomicAdd(a.count, sum);
    }
}

// meta_eval_batch_kernel: one launch of a planned batch (meta_batch_plan.h) — up to MB_MAX_PROGRAMS programs over a union table of up
// to MB_MAX_COLS columns, their answers written to any number of output bitmaps.  The shape is meta_eval_kernel's: a wave takes 64
// consecutive rows per step, a condition is one __ballot, the stack program folds wave-uniform masks.  What differs:
//   - a step reads each UNION column from global memory once, whatever the number of programs: first every column's tag, then numbers
//     and codes where the tag says so and some program of the launch tests them (need_num / need_code).  The tag loads of all
//     columns are issued before the first is consumed, and so are the number / code loads: the loops over the table are unrolled,
//     the first two only load, the third consumes;
//   - programs index columns by slot, so the per-lane values are staged in LDS (13 B x 64 lanes x 16 columns per wave) — in registers
//     that indexing would go through scratch.  A lane reads back only what it wrote itself: no barrier;
//   - the programs are an array in device memory, read at wave-uniform addresses, whole 32-bit words at a time.  progs, pairs, words, out and count are
//     __restrict__ parameters: the library's scratch block and the caller's outputs never overlap, and knowing it the compiler reads
//     programs and pairs with scalar loads;
//   - a step's answers (8 bytes per program) are parked in LDS, then written pair by pair, 8 pairs per wave instruction: lane =
//     (pair, byte), single bytes, so a row needs no alignment and nothing at or behind ceil(n / 8) of a row is touched;
//   - counts: lane p keeps program p's popcount over the wave's steps; after the loop the workgroup adds its waves' counts and issues
//     one atomic per pair, that is per output.
// Registers: the table's 48 pointers are loop-invariant, and so are the 48 lane masks hipcc makes of `slot u is in use / has its
// numbers tested / its codes tested`; kept in scalar registers across the row loop they spill.  So the pointers are held in vector
// registers, and the three bit sets pass through an empty asm in every step: the tests are redone per step from one VGPR each.
struct MetaBatchKernelArgs {
    const uint8_t *tag[MB_MAX_COLS]; // the union table
    const double *num[MB_MAX_COLS];
    const uint32_t *code[MB_MAX_COLS];
    uint32_t need_num, need_code; // bit u: some program of the launch tests the numbers / the codes of slot u
    uint32_t n_cols, n_prog, n_pairs;
    const uint8_t *valid, *extra; // optional bitmaps ANDed into every output, in this order
    uint64_t stride;
    uint64_t n;
};
// A program's 8- and 16-bit fields, read as part of an aligned 32-bit word at a wave-uniform address: the scalar unit has no narrower
// load, and a vector load of the same byte by all 64 lanes costs a trip to the vector cache per field.
__device__ __forceinline__ uint32_t meta_prog_bits(const uint32_t *pw, uint32_t byte_off, uint32_t mask) {
    return (pw[byte_off >> 2] >> (8 * (byte_off & 3))) & mask; // (a 16-bit field sits at an even offset: it never straddles words)
}
typedef const __attribute__((address_space(1))) uint8_t *meta_gp_u8;
typedef const __attribute__((address_space(1))) double *meta_gp_f64;
typedef const __attribute__((address_space(1))) uint32_t *meta_gp_u32;

__global__ void __launch_bounds__(64 * META_WAVES)
meta_eval_batch_kernel(const MetaBatchKernelArgs a, const MetaProgram *__restrict__ progs /* [n_prog] */,
                       const MetaBatchPair *__restrict__ pairs /* [n_pairs] */, const uint32_t *__restrict__ words, uint8_t *__restrict__ out,
                       uint32_t *__restrict__ count /* optional [outputs], zero at launch */) {
    __shared__ double s_num[META_WAVES][MB_MAX_COLS][64];
    __shared__ uint32_t s_code[META_WAVES][MB_MAX_COLS][64];
    __shared__ uint8_t s_tag[META_WAVES][MB_MAX_COLS][64];
    __shared__ unsigned long long cmask[META_WAVES][MP_MAX_CONDS];
    __shared__ unsigned long long stack[META_WAVES][MP_MAX_DEPTH + 1];
    __shared__ unsigned long long pres[META_WAVES][MB_MAX_PROGRAMS];
    __shared__ uint32_t pcount[META_WAVES][MB_MAX_PROGRAMS];
    const uint32_t lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); // (w: known to be wave-uniform)
    const uint64_t n_steps = (a.n + 63) / 64;
    uint64_t n_rows = a.n, n_bytes = (a.n + 7) / 8, stride = a.stride; // compared and multiplied per lane only: vector registers too
    asm volatile("" : "+v"(n_rows), "+v"(n_bytes), "+v"(stride));
    uint32_t allowed = 0; // of program `lane`
    uint64_t tag_p[MB_MAX_COLS], num_p[MB_MAX_COLS], code_p[MB_MAX_COLS];
#pragma unroll
    for (uint32_t u = 0; u < MB_MAX_COLS; u++) {
        tag_p[u] = (uint64_t)a.tag[u];
        num_p[u] = (uint64_t)a.num[u];
        code_p[u] = (uint64_t)a.code[u];
        asm volatile("" : "+v"(tag_p[u]), "+v"(num_p[u]), "+v"(code_p[u]));
    }
    uint32_t in_use = (1u << a.n_cols) - 1, need_num = a.need_num, need_code = a.need_code; // (n_cols <= 16)
    for (uint64_t g = (uint64_t)blockIdx.x * META_WAVES + w; g < n_steps; g += (uint64_t)gridDim.x * META_WAVES) {
        const uint64_t row = g * 64 + lane;
        bool ok = row < n_rows;
        if (ok && a.valid) ok = (a.valid[row >> 3] >> (row & 7)) & 1;
        if (ok && a.extra) ok = (a.extra[row >> 3] >> (row & 7)) & 1;
        const unsigned long long live = __ballot(ok);
        if (live) { // (wave-uniform)
            asm volatile("" : "+v"(in_use), "+v"(need_num), "+v"(need_code));
            const uint32_t load_tag = ok ? in_use : 0;
            uint32_t tag[MB_MAX_COLS];
            double num[MB_MAX_COLS];
            uint32_t code[MB_MAX_COLS];
#pragma unroll
            for (uint32_t u = 0; u < MB_MAX_COLS; u++) {
                tag[u] = LEANN_META_MISSING;
                if ((load_tag >> u) & 1) tag[u] = ((meta_gp_u8)tag_p[u])[row];
            }
#pragma unroll
            for (uint32_t u = 0; u < MB_MAX_COLS; u++) { // (a slot not in use, a row not ok: the tag is MISSING)
                num[u] = 0.0;
                code[u] = 0;
                if (tag[u] == LEANN_META_NUMBER && ((need_num >> u) & 1)) num[u] = ((meta_gp_f64)num_p[u])[row];
                if (tag[u] == LEANN_META_STRING && ((need_code >> u) & 1)) code[u] = ((meta_gp_u32)code_p[u])[row];
            }
#pragma unroll
            for (uint32_t u = 0; u < MB_MAX_COLS; u++)
                if ((in_use >> u) & 1) { // (the same in every lane)
                    s_tag[w][u][lane] = (uint8_t)tag[u];
                    s_num[w][u][lane] = num[u];   // 0 where the tag is not NUMBER or no program tests numbers
                    s_code[w][u][lane] = code[u]; // 0 where the tag is not STRING or no program tests codes
                }
            for (uint32_t p = 0; p < a.n_prog; p++) {
                const uint32_t *pw = reinterpret_cast<const uint32_t *>(progs + p);
                const uint32_t n_pcols = pw[offsetof(MetaProgram, n_cols) / 4], n_instr = pw[offsetof(MetaProgram, n_instr) / 4];
                for (uint32_t s = 0; s < n_pcols; s++) {
                    const uint32_t u = meta_prog_bits(pw, offsetof(MetaProgram, col_id) + 2 * s, 0xFFFF);
                    const uint32_t t = s_tag[w][u][lane];
                    const double x = s_num[w][u][lane];
                    const uint32_t c = s_code[w][u][lane];
                    const uint32_t i_end = meta_prog_bits(pw, offsetof(MetaProgram, col_first) + s + 1, 0xFF);
                    for (uint32_t i = meta_prog_bits(pw, offsetof(MetaProgram, col_first) + s, 0xFF); i < i_end; i++) {
                        union { MetaCond k; uint32_t w32[sizeof(MetaCond) / 4]; } cb;
#pragma unroll
                        for (uint32_t j = 0; j < sizeof(MetaCond) / 4; j++) cb.w32[j] = pw[offsetof(MetaProgram, cond) / 4 + i * (sizeof(MetaCond) / 4) + j];
                        cmask[w][i] = __ballot(meta_cond_test(cb.k, words, t, x, c));
                    }
                }
                // meta_run_program's loop (meta_plan.h), the instruction fetched as part of a word
                uint32_t sp = 0;
                stack[w][0] = 0;
                for (uint32_t i = 0; i < n_instr; i++) {
                    const uint32_t ins = meta_prog_bits(pw, offsetof(MetaProgram, instr) + 2 * i, 0xFFFF), op = ins >> 8, arg = ins & 0xFF;
                    switch (op) {
                    case MP_COND_AND: stack[w][sp] &= cmask[w][arg]; break;
                    case MP_COND_OR: stack[w][sp] |= cmask[w][arg]; break;
                    case MP_PUSH_AND: stack[w][++sp] = ~0ull; break;
                    case MP_PUSH_OR: stack[w][++sp] = 0; break;
                    case MP_FOLD_AND: sp--; stack[w][sp] &= stack[w][sp + 1]; break;
                    default: sp--; stack[w][sp] |= stack[w][sp + 1]; break;
                    }
                }
                const unsigned long long res = live & stack[w][0];
                pres[w][p] = res;
                if (lane == p) allowed += (uint32_t)__popcll(res);
            }
        }
        for (uint32_t j = lane >> 3; j < a.n_pairs; j += 8) { // (when nothing is live, zeros are still written)
            const MetaBatchPair pr = pairs[j];
            const unsigned long long res = live ? pres[w][pr.prog] : 0ull;
            const uint64_t byte = g * 8 + (lane & 7);
            if (byte < n_bytes) out[(uint64_t)pr.out * stride + byte] = (uint8_t)(res >> (8 * (lane & 7)));
        }
    }
    pcount[w][lane] = allowed;
    __syncthreads();
    if (count)
        for (uint32_t j = threadIdx.x; j < a.n_pairs; j += 64 * META_WAVES) {
            const MetaBatchPair pr = pairs[j];
            uint32_t sum = 0;
            for (int i = 0; i < META_WAVES; i++) sum += pcount[i][pr.prog];
            if (sum) atomicAdd(count + pr.out, sum);
        }
}

// ---- the store -----------------------------------------------------------------------------------------------------------------
extern "C" int leann_meta_create(size_t n, const uint8_t *valid, int device, leann_meta **out) {
    if (!out) { leann_set_error("leann_meta_create: null out"); return LEANN_ERR_INVALID; }
    *out = nullptr;
    if (n >= (1ull << 32)) { leann_set_error("leann_meta_create: n = %zu is 2^32 or more", n); return LEANN_ERR_INVALID; }
    if (int rc = leann_internal_check_device(device)) return rc;
    HIP_CHECK_RET(hipSetDevice(device));
    std::unique_ptr<leann_meta> m(new leann_meta());
    m->device = device;
    m->n = n;
    if (valid && n) {
        if (int rc = m->valid.alloc((n + 7) / 8)) return rc;
        HIP_CHECK_RET(hipMemcpy(m->valid, valid, (n + 7) / 8, hipMemcpyHostToDevice));
    }
    *out = m.release();
    return LEANN_OK;
}

extern "C" int leann_meta_add_column(leann_meta *m, const char *field, const uint8_t *tag, const double *num, const char *str_blob,
                                     const uint64_t *str_off) {
    if (!m || !field || (m->n && !tag)) { leann_set_error("leann_meta_add_column: null store, field or tag"); return LEANN_ERR_INVALID; }
    const size_t n = m->n;
    size_t n_num = 0, n_str = 0;
    for (size_t i = 0; i < n; i++) {
        if (tag[i] > LEANN_META_OTHER) {
            leann_set_error("leann_meta_add_column: tag[%zu] = %u is above LEANN_META_OTHER", i, (unsigned)tag[i]);
            return LEANN_ERR_INVALID;
        }
        n_num += tag[i] == LEANN_META_NUMBER;
        n_str += tag[i] == LEANN_META_STRING;
    }
    if (n_num && !num) { leann_set_error("leann_meta_add_column: %zu NUMBER rows but num is null", n_num); return LEANN_ERR_INVALID; }
    if (n_str && !str_off) { leann_set_error("leann_meta_add_column: %zu STRING rows but str_off is null", n_str); return LEANN_ERR_INVALID; }
    if (str_off) {
        for (size_t i = 0; i < n; i++)
            if (str_off[i + 1] < str_off[i]) {
                leann_set_error("leann_meta_add_column: str_off is not monotone at row %zu", i);
                return LEANN_ERR_INVALID;
            }
        if (n && str_off[n] > str_off[0] && !str_blob) { leann_set_error("leann_meta_add_column: str_off names bytes but str_blob is null"); return LEANN_ERR_INVALID; }
    }
    std::lock_guard<std::mutex> lk(m->mu);
    for (const auto &c : m->cols)
        if (c->field == field) { leann_set_error("leann_meta_add_column: duplicate field '%s'", field); return LEANN_ERR_INVALID; }
    if (m->cols.size() >= 65535) { leann_set_error("leann_meta_add_column: the store already holds 65535 columns"); return LEANN_ERR_INVALID; }
    try {
        std::unique_ptr<MetaColumn> col(new MetaColumn());
        col->field = field;
        // dictionary: the STRING rows ordered by their bytes (memcmp, a proper prefix first), then one sweep that numbers the distinct ones
        std::vector<uint32_t> codes;
        if (n_str) {
            std::vector<uint32_t> idx;
            idx.reserve(n_str);
            for (size_t i = 0; i < n; i++)
                if (tag[i] == LEANN_META_STRING) idx.push_back((uint32_t)i);
            auto cmp = [&](uint32_t x, uint32_t y) {
                const size_t lx = str_off[x + 1] - str_off[x], ly = str_off[y + 1] - str_off[y];
                const int c = memcmp(str_blob + str_off[x], str_blob + str_off[y], std::min(lx, ly));
                return c ? c : (lx < ly ? -1 : (lx > ly ? 1 : 0));
            };
            std::sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return cmp(x, y) < 0; });
            codes.assign(n, 0);
            for (size_t j = 0; j < idx.size(); j++) {
                if (j == 0 || cmp(idx[j - 1], idx[j]) != 0)
                    col->dict.emplace_back(str_blob + str_off[idx[j]], (size_t)(str_off[idx[j] + 1] - str_off[idx[j]]));
                codes[idx[j]] = (uint32_t)(col->dict.size() - 1);
            }
        }
        HIP_CHECK_RET(hipSetDevice(m->device));
        if (int rc = col->tag.alloc(n)) return rc;
        if (n) HIP_CHECK_RET(hipMemcpy(col->tag, tag, n, hipMemcpyHostToDevice));
        if (n_num) {
            if (int rc = col->num.alloc(n)) return rc;
            HIP_CHECK_RET(hipMemcpy(col->num, num, n * 8, hipMemcpyHostToDevice));
        }
        if (n_str) {
            if (int rc = col->code.alloc(n)) return rc;
            HIP_CHECK_RET(hipMemcpy(col->code, codes.data(), n * 4, hipMemcpyHostToDevice));
        }
        m->cols.push_back(std::move(col));
    } catch (const std::bad_alloc &) {
        leann_set_error("leann_meta_add_column: out of host memory building the dictionary");
        return LEANN_ERR_INVALID;
    }
    return LEANN_OK;
}

extern "C" int leann_meta_device_enabled(void) { return leann_knobs().meta_device ? 1 : 0; }
extern "C" size_t leann_meta_len(const leann_meta *m) { return m ? m->n : 0; }
extern "C" int leann_meta_has_column(const leann_meta *m, const char *field) {
    if (!m || !field) return 0;
    std::lock_guard<std::mutex> lk(m->mu);
    for (const auto &c : m->cols)
        if (c->field == field) return 1;
    return 0;
}
extern "C" void leann_meta_close(leann_meta *m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    (void)hipDeviceSynchronize(); // an evaluation on any stream may still be reading the columns
    delete m;
}

// ---- evaluation ----------------------------------------------------------------------------------------------------------------
// compile, then enqueue on `st` (m's device is current): d_count zeroed, sets / bitsets copied into the stream's block, the kernel
static int meta_enqueue(const leann_meta *m, const leann_meta_node *nodes, size_t n_nodes, const uint8_t *d_extra, uint8_t *d_out,
                        uint32_t *d_count, hipStream_t st) {
    MetaKernelArgs a{};
    std::vector<uint32_t> words;
    {
        std::lock_guard<std::mutex> lk(m->mu);
        std::vector<MetaColumnRef> refs;
        refs.reserve(m->cols.size());
        for (const auto &c : m->cols) refs.push_back(MetaColumnRef{c->field, &c->dict});
        std::string err;
        if (int rc = meta_compile(nodes, n_nodes, refs, &a.P, &words, &err)) {
            leann_set_error("%s", err.c_str());
            return rc;
        }
        for (uint32_t s = 0; s < a.P.n_cols; s++) {
            const MetaColumn &c = *m->cols[a.P.col_id[s]];
            a.tag[s] = c.tag;
            a.num[s] = c.num;   // null: no NUMBER row, never read
            a.code[s] = c.code; // null: no STRING row, never read
        }
        if (!words.empty()) {
            DeviceBuf<uint32_t> &blk = m->words[st]; // grows to the stream's largest filter; growing waits for the device
            if (int rc = blk.grow(words.size())) return rc;
            a.words = blk;
        }
    }
    // (pageable host memory: the call returns once `words` has been staged, and the copy is ordered on the stream behind the
    // previous evaluation's kernel, which read the same block — a copy of this kind cannot be captured into a graph)
    if (!words.empty()) HIP_CHECK_RET(hipMemcpyAsync(const_cast<uint32_t *>(a.words), words.data(), words.size() * 4, hipMemcpyHostToDevice, st));
    if (d_count) HIP_CHECK_RET(hipMemsetAsync(d_count, 0, 4, st));
    a.valid = m->valid;
    a.extra = d_extra;
    a.out = d_out;
    a.count = d_count;
    a.n = m->n;
    const uint64_t n_steps = (m->n + 63) / 64;
    const unsigned grid = (unsigned)std::min<uint64_t>(std::max<uint64_t>((n_steps + META_WAVES - 1) / META_WAVES, 1), META_MAX_GRID);
    hipLaunchKernelGGL(meta_eval_kernel, dim3(grid), dim3(64 * META_WAVES), 0, st, a);
    HIP_CHECK_RET(hipGetLastError());
    return LEANN_OK;
}

extern "C" int leann_meta_eval_device(const leann_meta *m, const leann_meta_node *nodes, size_t n_nodes, const uint8_t *d_and,
                                      uint8_t *d_bitmap, uint32_t *d_n_allowed, void *stream) {
    if (!m || !nodes || !d_bitmap) { leann_set_error("leann_meta_eval_device: null store, nodes or d_bitmap"); return LEANN_ERR_INVALID; }
    HIP_CHECK_RET(hipSetDevice(m->device));
    return meta_enqueue(m, nodes, n_nodes, d_and, d_bitmap, d_n_allowed, (hipStream_t)stream);
}

extern "C" int leann_meta_eval(const leann_meta *m, const leann_meta_node *nodes, size_t n_nodes, uint8_t *bitmap, size_t *n_allowed) {
    if (n_allowed) *n_allowed = 0;
    if (!m || !nodes || (m->n && !bitmap)) { leann_set_error("leann_meta_eval: null store, nodes or bitmap"); return LEANN_ERR_INVALID; }
    HIP_CHECK_RET(hipSetDevice(m->device));
    const size_t nbytes = (m->n + 7) / 8;
    DeviceBuf<uint8_t> d_out;
    DeviceBuf<uint32_t> d_count;
    if (int rc = d_out.alloc(nbytes)) return rc;
    if (int rc = d_count.alloc(1)) return rc;
    if (int rc = meta_enqueue(m, nodes, n_nodes, nullptr, d_out, d_count, nullptr)) return rc;
    uint32_t count = 0;
    if (nbytes) HIP_CHECK_RET(hipMemcpy(bitmap, d_out, nbytes, hipMemcpyDeviceToHost));
    HIP_CHECK_RET(hipMemcpy(&count, d_count, 4, hipMemcpyDeviceToHost));
    if (n_allowed) *n_allowed = count;
    return LEANN_OK;
}

extern "C" int leann_backend_filter_create_meta(const leann_backend *hc, const leann_meta *m, const leann_meta_node *nodes, size_t n_nodes,
                                                leann_filter **out) {
    if (!hc || !m || !nodes || !out) { leann_set_error("leann_backend_filter_create_meta: null argument"); return LEANN_ERR_INVALID; }
    *out = nullptr;
    if (m->n != hc->g.n) {
        leann_set_error("leann_backend_filter_create_meta: the store holds %zu rows, the index %zu", m->n, (size_t)hc->g.n);
        return LEANN_ERR_INVALID;
    }
    if (m->device != hc->device) {
        leann_set_error("leann_backend_filter_create_meta: the store is on device %d, the index on device %d", m->device, hc->device);
        return LEANN_ERR_INVALID;
    }
    if (hc->sharded) { // evaluated once on the store's device, then the per-shard registration of leann_backend_filter_create
        std::vector<uint8_t> bitmap(std::max<size_t>((m->n + 7) / 8, 1));
        if (int rc = leann_meta_eval(m, nodes, n_nodes, bitmap.data(), nullptr)) return rc;
        return leann_backend_filter_create(hc, bitmap.data(), out);
    }
    leann_filter *f = nullptr;
    if (int rc = leann_internal_filter_begin(hc, "leann_backend_filter_create_meta", &f)) return rc;
    int rc = meta_enqueue(m, nodes, n_nodes, nullptr, f->d_allow, nullptr, nullptr);
    if (rc == LEANN_OK && hipStreamSynchronize(nullptr) != hipSuccess) {
        leann_set_error("leann_backend_filter_create_meta: the evaluation failed on the device");
        rc = LEANN_ERR_DEVICE;
    }
    if (rc != LEANN_OK) { delete f; return rc; }
    return leann_internal_filter_finish(hc, f, out);
}

// ---- a batch of filters (meta_batch_plan.h) --------------------------------------------------------------------------------------
static int meta_batch_check_offsets(const char *who, const size_t *node_off, size_t n_out) {
    if (node_off[0] != 0) { leann_set_error("%s: node_off[0] = %zu, not 0", who, node_off[0]); return LEANN_ERR_INVALID; }
    for (size_t i = 0; i < n_out; i++)
        if (node_off[i + 1] < node_off[i]) { leann_set_error("%s: node_off is not monotone at filter %zu", who, i); return LEANN_ERR_INVALID; }
    return LEANN_OK;
}
// filters [0, n_out) planned against the store's dictionaries; host work only
static int meta_batch_make_plan(const leann_meta *m, const leann_meta_node *nodes, const size_t *node_off, size_t n_out, size_t index_base,
                                MetaBatchPlan *plan) {
    std::lock_guard<std::mutex> lk(m->mu);
    std::vector<MetaColumnRef> refs;
    refs.reserve(m->cols.size());
    for (const auto &c : m->cols) refs.push_back(MetaColumnRef{c->field, &c->dict});
    std::string err;
    try {
        if (int rc = meta_batch_plan(nodes, node_off, n_out, refs, plan, &err, index_base)) {
            leann_set_error("%s", err.c_str());
            return rc;
        }
    } catch (const std::bad_alloc &) {
        leann_set_error("metadata filters: out of host memory planning the batch");
        return LEANN_ERR_INVALID;
    }
    return LEANN_OK;
}
// enqueue a plan on `st` (m's device is current): the counters zeroed, ONE copy of every launch's programs, pairs and words into the
// stream's block, one kernel per launch.  Output i of the plan is d_out + i * stride and d_count[i].
static int meta_batch_enqueue(const leann_meta *m, const MetaBatchPlan &plan, size_t n_out, const uint8_t *d_extra, uint8_t *d_out,
                              size_t stride, uint32_t *d_count, hipStream_t st) {
    struct Piece { size_t progs, pairs, words; };
    std::vector<Piece> at(plan.launches.size());
    std::vector<unsigned char> blob;
    auto put = [&](const void *src, size_t bytes) { // at a 16-byte boundary
        blob.resize((blob.size() + 15) & ~(size_t)15);
        const size_t off = blob.size();
        blob.resize(off + bytes, 0);
        if (src && bytes) memcpy(blob.data() + off, src, bytes);
        return off;
    };
    for (size_t l = 0; l < plan.launches.size(); l++) {
        const MetaBatchLaunch &L = plan.launches[l];
        at[l].progs = put(L.programs.data(), L.programs.size() * sizeof(MetaProgram));
        at[l].pairs = put(L.pairs.data(), L.pairs.size() * sizeof(MetaBatchPair));
        at[l].words = put(L.words.data(), L.words.size() * 4);
    }
    std::vector<MetaBatchKernelArgs> args(plan.launches.size());
    unsigned char *base = nullptr;
    {
        std::lock_guard<std::mutex> lk(m->mu);
        DeviceBuf<unsigned char> &blk = m->batch[st]; // grows to the stream's largest batch; growing waits for the device
        if (int rc = blk.grow(blob.size())) return rc;
        base = blk;
        for (size_t l = 0; l < plan.launches.size(); l++) {
            const MetaBatchLaunch &L = plan.launches[l];
            MetaBatchKernelArgs &a = args[l];
            memset(&a, 0, sizeof a);
            for (size_t u = 0; u < L.cols.size(); u++) {
                const MetaColumn &c = *m->cols[L.cols[u]];
                a.tag[u] = c.tag;
                a.num[u] = c.num;   // null: no NUMBER row, never read
                a.code[u] = c.code; // null: no STRING row, never read
                a.need_num |= (uint32_t)(L.col_need[u] & 1) << u;
                a.need_code |= (uint32_t)((L.col_need[u] >> 1) & 1) << u;
            }
            a.n_cols = (uint32_t)L.cols.size();
            a.n_prog = (uint32_t)L.programs.size();
            a.n_pairs = (uint32_t)L.pairs.size();
        }
    }
    // (pageable host memory, as in meta_enqueue: the call returns once `blob` has been staged, and the copy is ordered on the stream
    // behind the previous batch's kernels, which read the same block)
    if (!blob.empty()) HIP_CHECK_RET(hipMemcpyAsync(base, blob.data(), blob.size(), hipMemcpyHostToDevice, st));
    if (d_count && n_out) HIP_CHECK_RET(hipMemsetAsync(d_count, 0, 4 * n_out, st));
    const uint64_t n_steps = (m->n + 63) / 64;
    const unsigned grid = (unsigned)std::min<uint64_t>(std::max<uint64_t>((n_steps + META_WAVES - 1) / META_WAVES, 1), META_MAX_GRID);
    for (size_t l = 0; l < args.size(); l++) {
        MetaBatchKernelArgs &a = args[l];
        a.valid = m->valid;
        a.extra = d_extra;
        a.stride = stride;
        a.n = m->n;
        hipLaunchKernelGGL(meta_eval_batch_kernel, dim3(grid), dim3(64 * META_WAVES), 0, st, a,
                           reinterpret_cast<const MetaProgram *>(base + at[l].progs), reinterpret_cast<const MetaBatchPair *>(base + at[l].pairs),
                           reinterpret_cast<const uint32_t *>(base + at[l].words), d_out, d_count);
        HIP_CHECK_RET(hipGetLastError());
    }
    return LEANN_OK;
}

extern "C" int leann_meta_eval_batch_device(const leann_meta *m, const leann_meta_node *nodes, const size_t *node_off, size_t n_out,
                                            const uint8_t *d_and, uint8_t *d_bitmaps, size_t stride, uint32_t *d_n_allowed,
                                            size_t *n_distinct, void *stream) {
    if (n_distinct) *n_distinct = 0;
    if (!m || !node_off || (n_out && (!nodes || !d_bitmaps))) {
        leann_set_error("leann_meta_eval_batch_device: null store, nodes, node_off or d_bitmaps");
        return LEANN_ERR_INVALID;
    }
    if (int rc = meta_batch_check_offsets("leann_meta_eval_batch_device", node_off, n_out)) return rc;
    if (n_out == 0) return LEANN_OK;
    if (stride < (m->n + 7) / 8) {
        leann_set_error("leann_meta_eval_batch_device: stride = %zu is below ceil(n / 8) = %zu", stride, (m->n + 7) / 8);
        return LEANN_ERR_INVALID;
    }
    if (n_out >= (1ull << 32)) { leann_set_error("leann_meta_eval_batch_device: n_out = %zu is 2^32 or more", n_out); return LEANN_ERR_INVALID; }
    MetaBatchPlan plan;
    if (int rc = meta_batch_make_plan(m, nodes, node_off, n_out, 0, &plan)) return rc;
    if (n_distinct) *n_distinct = plan.n_distinct;
    HIP_CHECK_RET(hipSetDevice(m->device));
    return meta_batch_enqueue(m, plan, n_out, d_and, d_bitmaps, stride, d_n_allowed, (hipStream_t)stream);
}

extern "C" int leann_meta_eval_batch(const leann_meta *m, const leann_meta_node *nodes, const size_t *node_off, size_t n_out,
                                     uint8_t *bitmaps, size_t stride, size_t *n_allowed, size_t *n_distinct) {
    if (n_distinct) *n_distinct = 0;
    if (!m || !node_off || (n_out && (!nodes || (m->n && !bitmaps)))) {
        leann_set_error("leann_meta_eval_batch: null store, nodes, node_off or bitmaps");
        return LEANN_ERR_INVALID;
    }
    if (int rc = meta_batch_check_offsets("leann_meta_eval_batch", node_off, n_out)) return rc;
    if (n_out == 0) return LEANN_OK;
    const size_t nbytes = (m->n + 7) / 8;
    if (stride < nbytes) {
        leann_set_error("leann_meta_eval_batch: stride = %zu is below ceil(n / 8) = %zu", stride, nbytes);
        return LEANN_ERR_INVALID;
    }
    if (n_out >= (1ull << 32)) { leann_set_error("leann_meta_eval_batch: n_out = %zu is 2^32 or more", n_out); return LEANN_ERR_INVALID; }
    MetaBatchPlan plan;
    if (int rc = meta_batch_make_plan(m, nodes, node_off, n_out, 0, &plan)) return rc;
    if (n_distinct) *n_distinct = plan.n_distinct;
    HIP_CHECK_RET(hipSetDevice(m->device));
    DeviceBuf<uint8_t> d_out;
    DeviceBuf<uint32_t> d_count;
    if (int rc = d_out.alloc(n_out * nbytes)) return rc;
    if (int rc = d_count.alloc(n_out)) return rc;
    if (int rc = meta_batch_enqueue(m, plan, n_out, nullptr, d_out, nbytes, d_count, nullptr)) return rc;
    if (nbytes) HIP_CHECK_RET(hipMemcpy2D(bitmaps, stride, d_out, nbytes, nbytes, n_out, hipMemcpyDeviceToHost));
    std::vector<uint32_t> counts(n_out);
    HIP_CHECK_RET(hipMemcpy(counts.data(), d_count, 4 * n_out, hipMemcpyDeviceToHost));
    if (n_allowed)
        for (size_t i = 0; i < n_out; i++) n_allowed[i] = counts[i];
    return LEANN_OK;
}

// nq queries, query i under filter i: the bitmaps of a chunk of queries are evaluated into library scratch, then the chunk is searched
// by the entry point a caller with those bitmaps would have used.  check: every argument and every filter, host work only — one plan
// per chunk; run: the device work.
struct MetaSearchPlan {
    size_t stride = 0, chunk = 0;
    std::vector<MetaBatchPlan> plans;
};
static int meta_search_check(const char *who, const leann_backend *hc, const leann_meta *m, const void *queries, size_t nq, size_t top_k,
                             const leann_meta_node *nodes, const size_t *node_off, int mode, const void *keys, const void *dists,
                             const void *counts, MetaSearchPlan *sp) {
    if (!hc || !m || !node_off || top_k == 0 || (nq && (!queries || !nodes || !keys || !dists || !counts))) {
        leann_set_error("%s: null/zero argument", who);
        return LEANN_ERR_INVALID;
    }
    if (mode != 0 && mode != 1) { leann_set_error("%s: mode = %d is neither 0 (walk) nor 1 (exact)", who, mode); return LEANN_ERR_INVALID; }
    if (m->n != hc->g.n) {
        leann_set_error("%s: the store holds %zu rows, the index %zu", who, m->n, (size_t)hc->g.n);
        return LEANN_ERR_INVALID;
    }
    if (m->device != hc->device) {
        leann_set_error("%s: the store is on device %d, the index on device %d", who, m->device, hc->device);
        return LEANN_ERR_INVALID;
    }
    if (int rc = meta_batch_check_offsets(who, node_off, nq)) return rc;
    sp->stride = std::max<size_t>(((m->n + 7) / 8 + 15) & ~(size_t)15, 16);
    const size_t budget = leann_knobs().meta_batch_bytes ? (size_t)leann_knobs().meta_batch_bytes : (size_t)1 << 30;
    sp->chunk = std::max<size_t>(1, std::min(nq, std::max<size_t>(1, budget / sp->stride)));
    sp->plans.resize((nq + sp->chunk - 1) / sp->chunk);
    for (size_t c = 0; c < sp->plans.size(); c++) {
        const size_t q0 = c * sp->chunk, k = std::min(sp->chunk, nq - q0);
        std::vector<size_t> off(node_off + q0, node_off + q0 + k + 1);
        for (size_t &o : off) o -= node_off[q0];
        if (int rc = meta_batch_make_plan(m, nodes + node_off[q0], off.data(), k, q0, &sp->plans[c])) return rc;
    }
    return LEANN_OK;
}
static int meta_search_run(const char *who, const leann_backend *hc, const leann_meta *m, const MetaSearchPlan &sp, const float *d_queries,
                           size_t nq, size_t top_k, size_t complexity, int mode, uint64_t *d_keys, float *d_dists, uint32_t *d_counts,
                           uint32_t *d_stats, uint32_t *d_n_allowed, hipStream_t st) {
    if (nq == 0) return LEANN_OK;
    HIP_CHECK_RET(hipSetDevice(m->device));
    ScratchLease<uint8_t> bitmaps;
    if (int rc = bitmaps.acquire(sp.chunk * sp.stride)) return rc;
    const size_t d = hc->g.d;
    int rc = LEANN_OK;
    for (size_t c = 0; c < sp.plans.size() && rc == LEANN_OK; c++) {
        const size_t q0 = c * sp.chunk, k = std::min(sp.chunk, nq - q0);
        rc = meta_batch_enqueue(m, sp.plans[c], k, nullptr, bitmaps, sp.stride, d_n_allowed ? d_n_allowed + q0 : nullptr, st);
        if (rc == LEANN_OK)
            rc = mode == 0 ? leann_backend_search_filtered_batch_device(hc, d_queries + q0 * d, k, top_k, complexity, bitmaps, sp.stride,
                                                                        d_keys + q0 * top_k, d_dists + q0 * top_k, d_counts + q0,
                                                                        d_stats ? d_stats + q0 * 4 : nullptr, st)
                           : leann_backend_search_filtered_exact_batch_device(hc, d_queries + q0 * d, k, top_k, bitmaps, sp.stride,
                                                                              d_keys + q0 * top_k, d_dists + q0 * top_k, d_counts + q0, st);
        // the next chunk overwrites the bitmaps, and the lease ends with the call: nothing may still be reading them
        if (hipStreamSynchronize(st) != hipSuccess && rc == LEANN_OK) {
            leann_set_error("%s: the evaluation or the search failed on the device", who);
            rc = LEANN_ERR_DEVICE;
        }
    }
    return rc;
}

extern "C" int leann_backend_search_meta_batch_device(const leann_backend *hc, const leann_meta *m, const float *d_queries, size_t nq,
                                                      size_t top_k, size_t complexity, const leann_meta_node *nodes, const size_t *node_off,
                                                      int mode, uint64_t *d_keys, float *d_dists, uint32_t *d_counts, uint32_t *d_stats,
                                                      uint32_t *d_n_allowed, void *stream) {
    const char *who = "leann_backend_search_meta_batch_device";
    MetaSearchPlan sp;
    if (int rc = meta_search_check(who, hc, m, d_queries, nq, top_k, nodes, node_off, mode, d_keys, d_dists, d_counts, &sp)) return rc;
    return meta_search_run(who, hc, m, sp, d_queries, nq, top_k, complexity, mode, d_keys, d_dists, d_counts, d_stats, d_n_allowed,
                           (hipStream_t)stream);
}

extern "C" int leann_backend_search_meta_batch(const leann_backend *hc, const leann_meta *m, const float *queries, size_t nq, size_t top_k,
                                               size_t complexity, const leann_meta_node *nodes, const size_t *node_off, int mode,
                                               uint64_t *keys, float *dists, uint32_t *counts, uint32_t *stats, uint32_t *n_allowed) {
    const char *who = "leann_backend_search_meta_batch";
    MetaSearchPlan sp;
    if (int rc = meta_search_check(who, hc, m, queries, nq, top_k, nodes, node_off, mode, keys, dists, counts, &sp)) return rc;
    if (nq == 0) return LEANN_OK;
    HIP_CHECK_RET(hipSetDevice(hc->device));
    const size_t d = hc->g.d;
    DeviceBuf<float> d_q, d_dists;
    DeviceBuf<uint64_t> d_keys;
    DeviceBuf<uint32_t> d_counts, d_stats, d_allowed;
    if (int rc = d_q.alloc(nq * d)) return rc;
    if (int rc = d_keys.alloc(nq * top_k)) return rc;
    if (int rc = d_dists.alloc(nq * top_k)) return rc;
    if (int rc = d_counts.alloc(nq)) return rc;
    if (int rc = d_stats.alloc(nq * 4)) return rc;
    if (int rc = d_allowed.alloc(nq)) return rc;
    HIP_CHECK_RET(hipMemcpy(d_q, queries, nq * d * 4, hipMemcpyHostToDevice));
    HIP_CHECK_RET(hipMemset(d_stats, 0, nq * 16));
    if (int rc = meta_search_run(who, hc, m, sp, d_q, nq, top_k, complexity, mode, d_keys, d_dists, d_counts, d_stats, d_allowed, nullptr)) return rc;
    HIP_CHECK_RET(hipMemcpy(keys, d_keys, nq * top_k * 8, hipMemcpyDeviceToHost));
    HIP_CHECK_RET(hipMemcpy(dists, d_dists, nq * top_k * 4, hipMemcpyDeviceToHost));
    HIP_CHECK_RET(hipMemcpy(counts, d_counts, nq * 4, hipMemcpyDeviceToHost));
    if (stats) HIP_CHECK_RET(hipMemcpy(stats, d_stats, nq * 16, hipMemcpyDeviceToHost));
    if (n_allowed) HIP_CHECK_RET(hipMemcpy(n_allowed, d_allowed, nq * 4, hipMemcpyDeviceToHost));
    return LEANN_OK;
}
