// narrow_rows.h — what a narrow row type is (LEANN_ROWS_BF16, LEANN_ROWS_I8; include/leann_backend.h "row types"), and the one row store
// every such type shares (narrow_rows.hip).  Included by internal.h.
//
// A narrow index stores its vectors in a type of fewer than four bytes and is, by definition, the f32 index over the widened rows with
// the same graph, bit for bit.  g.X names the handle's own store, [n x g.row_bytes] bytes, every row whole 128-B lines, zero padded,
// the elements in the type's own order; g.ld keeps the f32 meaning (dims rounded up to 4) and selects the kernel; g.feat_h stays 0;
// no f32 rows exist and no planes are ever cut.  Files and exports hold the rows in plain element order.
//
// A further row type takes one NarrowRows beside its encode kernel, named in leann_internal_narrow; one search unit; one file version.
#pragma once
#include <functional>
#include <stdint.h>
#include <vector>

// f32 device rows [m x ld] — `row0`: the index of the first in the whole matrix — handed to a per-slab function; a SlabLoop hands every
// slab of a matrix to the function it is given, in order, and stops at the first non-zero return.
using SlabFn = std::function<int(float *d_rows, size_t m, size_t row0)>;
using SlabLoop = std::function<int(const SlabFn &)>;

struct NarrowRows {
    int row_type;          // LEANN_ROWS_*
    const char *name;      // as the messages print it
    uint32_t elem_bytes;
    uint32_t file_version; // of the index file that holds such rows
    uint32_t (*store_pitch)(uint32_t dims);       // bytes of a store row
    uint32_t (*pos)(uint32_t j, uint32_t ld);     // where element j sits in its store row of ld elements: a permutation of [0, ld)
    // null, or what the encoding needs to know of ALL rows before the first is encoded (int8: the column exponents, *exps [d]), from a
    // pass over the rows [.. x ld]; `who` names the entry point in the refusal of a row that cannot be encoded
    int (*fit)(const char *who, uint32_t d, uint32_t ld, const SlabLoop &each_slab, std::vector<int8_t> *exps);
    // f32 device rows [m x ld] (ld a multiple of 4, >= d) -> store rows at `store` (may be null); write_back: the narrowed values,
    // widened again, over the source.  exps: what fit gave.  Every byte of a store row is written, padding as zero.
    int (*encode)(float *d_rows, size_t m, uint32_t d, size_t ld, const int8_t *exps, void *store, bool write_back);
    // `count` elements of rows [.. x d] in element order -> f32 at dst, exact, front to back; dst may overlap src the way
    // leann_backend_graph_export arranges it
    void (*widen)(const unsigned char *src, size_t count, size_t d, const int8_t *exps, unsigned char *dst);
};
const NarrowRows *leann_internal_bf16_rows(), *leann_internal_i8_rows();  // rows_bf16.hip, rows_i8.hip
const NarrowRows *leann_internal_narrow(int row_type);                    // null for LEANN_ROWS_F32 and for anything unknown
const NarrowRows *leann_internal_narrow_of_version(uint32_t file_version); // null for a version that holds no narrow rows

// Where a new narrow handle's rows come from, other than host f32 rows: an index file's rows [n x dims] in element order and the
// handle's own type (int8: with the file's column exponents, exps [dims]), or f32 rows on the device, d_f32 [n x d_ld].
struct NarrowSource {
    const void *file_rows;
    const int8_t *exps;
    const float *d_f32;
    size_t d_ld;
};

struct leann_backend;
// Allocate h's store (h->g.n / d / ld set; h's device current) and fill it from host f32 rows [n x d] — through a transient device
// slab of at most 256 MiB, encoded by the same kernel as every other way in — or from `src`; exactly one source when n != 0.
// Afterwards h owns the store and names no f32 rows.  Exponents h already has (a device build's) are kept.
int leann_internal_narrow_adopt(leann_backend *h, const NarrowRows *t, const float *host_f32, const NarrowSource &src, const char *who);
// store rows [r0, r0 + rows) as [rows x d] of the handle's type in element order
int leann_internal_narrow_to_host(const leann_backend *h, size_t r0, size_t rows, void *out);
// rows_i8.hip: the column scales 2^-e_j of h->i8_exps on the device (f32 [g.ld], padding 1.0; g.norms), and what is wrong, if
// anything, with an index file's exponents and codes
int leann_internal_i8_bind_scales(leann_backend *h);
const char *leann_internal_i8_check_file_rows(const int8_t *exps, const int8_t *codes, size_t n, size_t d);
