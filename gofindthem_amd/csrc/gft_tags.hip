// gft_tags.hip -- leaf hit bitmap of a record batch -> per-record lists of (field, expression): the batch form of TagObject's
// map (group/finder/finder.go:87-110, internal.go:9-38), gfx950 / wave64.
//
//   hit rows [n_leaves][W] (W = ceil(n_exprs / 32)), leaf_field [n_leaves], rec_off [n_records + 1], valid [ceil(F / 32)]  ->
//   row_off [n_records + 1] u64, ent_field / ent_expr / ent_tag [total] u32: leaves in record order, expressions ascending
//   inside a leaf
//
//   k_tags<false>  popcount per leaf row, the row taken as zero when the leaf's field is invalid or outside the schema
//                                                                                   -> cnt [n_leaves] u32
//   (k_scan_partials / k_scan_spine / k_scan_final of gft_kernels.hip: cnt -> leaf_ent_off [n_leaves + 1])
//   k_tags<true>   row_off[r] = leaf_ent_off[rec_off[r]], every word once with a plain store; then every set bit of a
//                  contributing leaf's row, lowest first, from leaf_ent_off[leaf] on
//
// The walk over the rows is walk_bit_rows (gft_bitrows_dev.hpp), a row a leaf, its key the leaf's field: a leaf that does
// not contribute has none and its row is not read.  Nothing is stored at or past `cap` entries.  The passes also validate
// what they read: a field index outside the schema sets flags[0] (count pass), record offsets that descend, leave
// [0, n_leaves] or do not end at n_leaves set flags[1] (fill pass) -- plain stores of 1; such leaves count nothing and such
// offsets are never used as an index.  Memory bound: two reads of the bitmap plus the output.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gft_tags.hpp"

namespace gft {

namespace {

template <bool FILL>
struct TagSink {
    const TagParams& P;
    // the field of a leaf when the leaf contributes
    __device__ __forceinline__ uint32_t key(uint64_t leaf, bool first) const {
        const uint32_t f = P.leaf_field[leaf];
        if (f >= P.n_fields) {
            if (!FILL && first) P.flags[0] = 1;
            return kNoKey;
        }
        return (P.valid[f >> 5] >> (f & 31) & 1u) ? f : kNoKey;
    }
    __device__ __forceinline__ void count(uint64_t leaf, uint32_t c) const { P.cnt[leaf] = c; }
    __device__ __forceinline__ uint64_t base(uint64_t leaf) const { return P.leaf_ent_off[leaf]; }
    __device__ __forceinline__ void emit(uint32_t field, uint32_t x, uint64_t pos) const {
        if (pos < P.cap) {
            P.ent_expr[pos] = x;
            P.ent_field[pos] = field;
            if (P.ent_tag) P.ent_tag[pos] = P.expr_tag[x];
        }
    }
};

template <bool FILL>
__global__ void __launch_bounds__(kBitRowsBlock) k_tags(const TagParams P) {
    const uint64_t tid = (uint64_t)blockIdx.x * kBitRowsBlock + threadIdx.x;
    const uint64_t n_threads = (uint64_t)gridDim.x * kBitRowsBlock;
    const uint64_t n_leaves = P.rows.n_rows;
    if (FILL) {
        // the records' offsets into the entries, gathered through rec_off once that is known to be an index
        for (uint64_t r = tid; r <= P.n_records; r += n_threads) {
            const uint64_t o = P.rec_off[r];
            const bool last = r == P.n_records;
            if (o > n_leaves || (last ? o != n_leaves : P.rec_off[r + 1] < o)) P.flags[1] = 1;
            P.row_off[r] = o <= n_leaves ? P.leaf_ent_off[o] : 0;
        }
        if (!P.cap || !P.rows.W) return;
    } else if (!P.rows.W) {                          // a finder without expressions: nothing to count, the fields are still checked
        for (uint64_t l = tid; l < n_leaves; l += n_threads) {
            if (P.leaf_field[l] >= P.n_fields) P.flags[0] = 1;
            P.cnt[l] = 0;
        }
        return;
    }
    walk_bit_rows<FILL>(P.rows, TagSink<FILL>{P});
}

// beside the walk: W == 0, a thread a leaf; the fill pass, a thread a row_off word
unsigned tags_grid(const TagParams& P, uint64_t n_gather, unsigned n_cus) {
    const uint64_t per_leaf = P.rows.W ? 0 : (P.rows.n_rows + kBitRowsBlock - 1) / kBitRowsBlock;
    return bit_rows_grid(P.rows, n_cus, std::max(per_leaf, (n_gather + kBitRowsBlock - 1) / kBitRowsBlock));
}

}  // namespace

hipError_t launch_tags_count(const TagParams& P, unsigned n_cus, hipStream_t st) {
    if (!P.rows.n_rows) return hipSuccess;
    k_tags<false><<<dim3(tags_grid(P, 0, n_cus)), dim3(kBitRowsBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_tags_fill(const TagParams& P, unsigned n_cus, hipStream_t st) {
    k_tags<true><<<dim3(tags_grid(P, P.n_records + 1, n_cus)), dim3(kBitRowsBlock), 0, st>>>(P);
    return hipGetLastError();
}

}  // namespace gft
