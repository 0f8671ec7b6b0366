// gft_compact.hip -- hit bitmap -> per-document lists of true expressions (the batch form of []ExpressionResult,
// finder/finder.go:25-29, 199-215), gfx950 / wave64.
//
//   bitmap [n_docs][W] (W = ceil(n_exprs / 32), layout of gft_process)  ->
//   row_off [n_docs + 1] u64, expr_idx [total] u32 ascending inside a document, label [total] u32 (optional)
//
//   k_compact<false>  popcount per row                                         -> cnt [n_docs] u32
//   (k_scan_partials / k_scan_spine / k_scan_final of gft_kernels.hip: cnt -> row_off)
//   k_compact<true>   exclusive prefix of the word popcounts inside a row, then every lane writes the set bits of
//                     its word, lowest first, at row_off[row] + prefix
//
// Both passes read the bitmap with the lanes of a wave on consecutive words.  W <= 64: a wave takes 64 / W' rows at
// once (W' = W rounded up to a power of two; a row is a segment of W' lanes, the lanes W..W'-1 of a segment idle) and
// reduces / scans per segment with shuffles.  W > 64: a wave walks one row in steps of 64 words with a carry.  W is a
// run-time value.  Nothing is stored at or past `cap` entries; bits at and above n_exprs in a row's last word are
// masked.  Memory bound: two reads of the bitmap plus the output.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gft_kernels.hpp"

namespace gft {

namespace {

constexpr uint32_t kCompactBlock = 256;     // 4 waves
constexpr uint32_t kCompactUnroll = 4;      // row groups a wave has in flight (W <= 64): four loads before the first use

struct CompactParams {
    const uint32_t* bitmap;
    uint64_t n_docs;
    uint32_t W, lg;                 // words per row; W <= 64: W' = 1 << lg
    uint32_t tail;                  // valid bits of a row's last word
    uint32_t* cnt;                  // count pass
    const uint64_t* row_off;        // fill pass
    uint32_t* expr_idx;
    uint32_t* label;                // nullable
    const uint32_t* expr_label;     // [n_exprs] when label != nullptr
    uint64_t cap;
};

// the set bits of word j of a row, lowest first, to positions pos, pos + 1, ...
__device__ __forceinline__ void write_bits(const CompactParams& P, uint32_t w, uint32_t j, uint64_t pos) {
    while (w) {
        const uint32_t x = j * 32u + (uint32_t)__builtin_ctz(w);
        w &= w - 1;
        if (pos < P.cap) {
            P.expr_idx[pos] = x;
            if (P.label) P.label[pos] = P.expr_label[x];
        }
        pos++;
    }
}

template <bool FILL>
__global__ void __launch_bounds__(kCompactBlock) k_compact(const CompactParams P) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * kCompactBlock + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * kCompactBlock) >> 6;
    const uint32_t W = P.W;
    if (W <= 64) {
        const uint32_t Wp = 1u << P.lg, R = 64u >> P.lg;
        const uint32_t seg = lane >> P.lg, j = lane & (Wp - 1);
        const uint64_t n_groups = (P.n_docs + R - 1) / R;
        const uint32_t mask = j + 1 == W ? P.tail : 0xFFFFFFFFu;
        for (uint64_t g = wave * kCompactUnroll; g < n_groups; g += n_waves * kCompactUnroll) {
            uint32_t w[kCompactUnroll];
#pragma unroll
            for (uint32_t u = 0; u < kCompactUnroll; u++) {
                const uint64_t row = (g + u) * R + seg;
                w[u] = (j < W && row < P.n_docs) ? P.bitmap[row * W + j] & mask : 0u;
            }
#pragma unroll
            for (uint32_t u = 0; u < kCompactUnroll; u++) {
                if (g + u >= n_groups) break;                       // (the same in every lane)
                const uint64_t row = (g + u) * R + seg;
                const uint32_t c = (uint32_t)__builtin_popcount(w[u]);
                uint32_t v = c;
                if (!FILL) {
                    for (uint32_t s = 1; s < Wp; s <<= 1) v += __shfl_xor(v, (int)s, 64);
                    if (j == 0 && row < P.n_docs) P.cnt[row] = v;
                } else {
                    for (uint32_t s = 1; s < Wp; s <<= 1) {
                        const uint32_t o = __shfl_up(v, s, 64);
                        if (j >= s) v += o;
                    }
                    if (w[u]) write_bits(P, w[u], j, P.row_off[row] + (v - c));   // (w != 0: j < W and row < n_docs)
                }
            }
        }
    } else {
        for (uint64_t row = wave; row < P.n_docs; row += n_waves) {
            const uint32_t* r = P.bitmap + row * W;
            uint64_t carry = FILL ? P.row_off[row] : 0;
            uint32_t acc = 0;
            for (uint32_t k = 0; k < W; k += 64) {
                const uint32_t j = k + lane;
                const uint32_t w = j < W ? r[j] & (j + 1 == W ? P.tail : 0xFFFFFFFFu) : 0u;
                const uint32_t c = (uint32_t)__builtin_popcount(w);
                if (!FILL) {
                    acc += c;
                } else {
                    uint32_t v = c;
#pragma unroll
                    for (uint32_t s = 1; s < 64; s <<= 1) {
                        const uint32_t o = __shfl_up(v, s, 64);
                        if (lane >= s) v += o;
                    }
                    if (w) write_bits(P, w, j, carry + (v - c));
                    carry += __shfl(v, 63, 64);
                }
            }
            if (!FILL) {
#pragma unroll
                for (uint32_t s = 1; s < 64; s <<= 1) acc += __shfl_xor(acc, (int)s, 64);
                if (lane == 0) P.cnt[row] = acc;
            }
        }
    }
}

CompactParams compact_params(const uint32_t* d_bitmap, uint64_t n_docs, uint32_t n_exprs) {
    CompactParams P{};
    P.bitmap = d_bitmap;
    P.n_docs = n_docs;
    P.W = (n_exprs + 31) / 32;
    while ((1u << P.lg) < P.W && P.lg < 6) P.lg++;
    P.tail = (n_exprs & 31) ? (1u << (n_exprs & 31)) - 1 : 0xFFFFFFFFu;
    return P;
}

unsigned compact_grid(const CompactParams& P, unsigned n_cus) {
    // waves that have work: a group of 64 / W' rows per wave and trip (W <= 64), a row per wave otherwise
    const uint64_t items = P.W <= 64 ? (P.n_docs + (64u >> P.lg) - 1) / (64u >> P.lg) : P.n_docs;
    const uint64_t per_wave = P.W <= 64 ? kCompactUnroll : 1;
    const uint64_t blocks = (items + per_wave * (kCompactBlock / 64) - 1) / (per_wave * (kCompactBlock / 64));
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)std::max(n_cus, 1u) * 8));   // 32 waves per CU
}

}  // namespace

hipError_t launch_compact_count(const uint32_t* d_bitmap, uint64_t n_docs, uint32_t n_exprs, uint32_t* d_cnt, unsigned n_cus,
                                hipStream_t st) {
    if (!n_docs || !n_exprs) return hipSuccess;
    CompactParams P = compact_params(d_bitmap, n_docs, n_exprs);
    P.cnt = d_cnt;
    k_compact<false><<<dim3(compact_grid(P, n_cus)), dim3(kCompactBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_compact_fill(const uint32_t* d_bitmap, uint64_t n_docs, uint32_t n_exprs, const uint64_t* d_row_off,
                               uint32_t* d_expr_idx, uint32_t* d_label, const uint32_t* d_expr_label, uint64_t cap, unsigned n_cus,
                               hipStream_t st) {
    if (!n_docs || !n_exprs || !cap) return hipSuccess;
    CompactParams P = compact_params(d_bitmap, n_docs, n_exprs);
    P.row_off = d_row_off;
    P.expr_idx = d_expr_idx;
    P.label = d_label;
    P.expr_label = d_expr_label;
    P.cap = cap;
    k_compact<true><<<dim3(compact_grid(P, n_cus)), dim3(kCompactBlock), 0, st>>>(P);
    return hipGetLastError();
}

}  // namespace gft
