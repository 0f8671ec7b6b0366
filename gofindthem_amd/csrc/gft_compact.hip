// gft_compact.hip -- hit bitmap -> per-document lists of true expressions (the batch form of []ExpressionResult,
// finder/finder.go:25-29, 199-215), gfx950 / wave64.
//
//   bitmap [n_docs][W] (W = ceil(n_exprs / 32), layout of gft_process)  ->
//   row_off [n_docs + 1] u64, expr_idx [total] u32 ascending inside a document, label [total] u32 (optional)
//
//   k_compact<false>  popcount per row                                         -> cnt [n_docs] u32
//   (k_scan_partials / k_scan_spine / k_scan_final of gft_kernels.hip: cnt -> row_off)
//   k_compact<true>   every set bit of a row, lowest first, from row_off[row] on
//
// The walk over the rows is walk_bit_rows (gft_bitrows_dev.hpp), a row a document and every row with a key.  Nothing is
// stored at or past `cap` entries.  Memory bound: two reads of the bitmap plus the output.
#include <hip/hip_runtime.h>

#include "gft_bitrows_dev.hpp"
#include "gft_kernels.hpp"

namespace gft {

namespace {

struct CompactParams {
    BitRows rows;                   // a row a document
    uint32_t* cnt;                  // count pass
    const uint64_t* row_off;        // fill pass
    uint32_t* expr_idx;
    uint32_t* label;                // nullable
    const uint32_t* expr_label;     // [n_exprs] when label != nullptr
    uint64_t cap;
};

struct CompactSink {
    const CompactParams& P;
    __device__ __forceinline__ uint32_t key(uint64_t, bool) const { return 0; }
    __device__ __forceinline__ void count(uint64_t row, uint32_t c) const { P.cnt[row] = c; }
    __device__ __forceinline__ uint64_t base(uint64_t row) const { return P.row_off[row]; }
    __device__ __forceinline__ void emit(uint32_t, uint32_t x, uint64_t pos) const {
        if (pos < P.cap) {
            P.expr_idx[pos] = x;
            if (P.label) P.label[pos] = P.expr_label[x];
        }
    }
};

template <bool FILL>
__global__ void __launch_bounds__(kBitRowsBlock) k_compact(const CompactParams P) {
    walk_bit_rows<FILL>(P.rows, CompactSink{P});
}

}  // namespace

hipError_t launch_compact_count(const uint32_t* d_bitmap, uint64_t n_docs, uint32_t n_exprs, uint32_t* d_cnt, unsigned n_cus,
                                hipStream_t st) {
    if (!n_docs || !n_exprs) return hipSuccess;
    CompactParams P{};
    P.rows = bit_rows(d_bitmap, n_docs, n_exprs);
    P.cnt = d_cnt;
    k_compact<false><<<dim3(bit_rows_grid(P.rows, n_cus, 0)), dim3(kBitRowsBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_compact_fill(const uint32_t* d_bitmap, uint64_t n_docs, uint32_t n_exprs, const uint64_t* d_row_off,
                               uint32_t* d_expr_idx, uint32_t* d_label, const uint32_t* d_expr_label, uint64_t cap, unsigned n_cus,
                               hipStream_t st) {
    if (!n_docs || !n_exprs || !cap) return hipSuccess;
    CompactParams P{};
    P.rows = bit_rows(d_bitmap, n_docs, n_exprs);
    P.row_off = d_row_off;
    P.expr_idx = d_expr_idx;
    P.label = d_label;
    P.expr_label = d_expr_label;
    P.cap = cap;
    k_compact<true><<<dim3(bit_rows_grid(P.rows, n_cus, 0)), dim3(kBitRowsBlock), 0, st>>>(P);
    return hipGetLastError();
}

}  // namespace gft
