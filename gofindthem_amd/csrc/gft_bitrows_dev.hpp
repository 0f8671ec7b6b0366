// gft_bitrows_dev.hpp -- the walk over the rows of a hit bitmap that the sparse outputs share (gft_compact.hip: a row a
// document; gft_tags.hip: a row a leaf), gfx950 / wave64.  For .hip files; gft_tags.hpp brings it along for BitRows.
//
//   bitmap [n_rows][W] (W = ceil(n_exprs / 32), layout of gft_process)
//
//   walk_bit_rows<false>  popcount per row                                      -> Sink::count(row, c)
//   walk_bit_rows<true>   exclusive prefix of the word popcounts inside a row, then every lane hands the set bits of its
//                         word, lowest first, to Sink::emit(key, x, Sink::base(row) + prefix ...)
//   join_bit_rows         an arbitrary value per word joined over the row (gft_select.hip, gft_route.hip): at the end of this file
//
// Both passes read the bitmap with the lanes of a wave on consecutive words.  W <= 64: a wave takes 64 / W' rows at once
// (W' = W rounded up to a power of two; a row is a segment of W' lanes, the lanes W..W'-1 of a segment idle) and reduces /
// scans per segment with shuffles, kBitRowsUnroll groups in flight.  W > 64: a wave walks one row in steps of 64 words with
// a carry.  W is a run-time value, W == 0 is the caller's.  Bits at and above n_exprs in a row's last word are masked.
//
// The sink is a small struct around the kernel's parameter block:
//   uint32_t key(row, first)  a value carried to emit, asked once per lane and row < n_rows before the row's words are
//                             loaded; kNoKey: the row contributes nothing and is not loaded.  `first`: the one lane of the
//                             row that may store (the lane that also calls count)
//   void count(row, c)        count pass, every row once -- c = 0 for a row without a key
//   uint64_t base(row)        fill pass: where the row's entries begin
//   void emit(key, x, pos)    fill pass: bit x of the row is entry pos (the test against the cap is the sink's)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "gft_bitrows.hpp"
#include "gft_wave_dev.hpp"

namespace gft {

constexpr uint32_t kBitRowsBlock = 256;     // 4 waves
constexpr uint32_t kBitRowsUnroll = 4;      // row groups a wave has in flight (W <= 64): four loads before the first use
constexpr uint32_t kNoKey = 0xFFFFFFFFu;

struct BitRows {
    const uint32_t* bitmap;         // [n_rows][W]
    uint64_t n_rows;
    uint32_t W, lg;                 // words per row; W <= 64: W' = 1 << lg
    uint32_t tail;                  // valid bits of a row's last word
};

inline BitRows bit_rows(const uint32_t* d_bitmap, uint64_t n_rows, uint32_t n_exprs) {
    BitRows B{};
    B.bitmap = d_bitmap;
    B.n_rows = n_rows;
    B.W = (n_exprs + 31) / 32;
    B.lg = bit_row_lg(B.W);
    B.tail = (n_exprs & 31) ? (1u << (n_exprs & 31)) - 1 : 0xFFFFFFFFu;
    return B;
}

// blocks of kBitRowsBlock threads; min_blocks: what the kernel does beside the walk, a thread an item
inline unsigned bit_rows_grid(const BitRows& B, unsigned n_cus, uint64_t min_blocks) {
    // waves that have work: a group of 64 / W' rows per wave and trip (W <= 64), a row per wave otherwise
    const uint64_t items = B.W <= 64 ? (B.n_rows + (64u >> B.lg) - 1) / (64u >> B.lg) : B.n_rows;
    const uint64_t per_wave = B.W <= 64 ? kBitRowsUnroll : 1;
    const uint64_t blocks = std::max((items + per_wave * (kBitRowsBlock / 64) - 1) / (per_wave * (kBitRowsBlock / 64)), min_blocks);
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)std::max(n_cus, 1u) * 8));   // 32 waves per CU
}

// the set bits of word j of a row, lowest first, to positions pos, pos + 1, ...
template <class Sink>
__device__ __forceinline__ void emit_bits(const Sink& S, uint32_t key, uint32_t w, uint32_t j, uint64_t pos) {
    while (w) {
        S.emit(key, j * 32u + (uint32_t)__builtin_ctz(w), pos);
        w &= w - 1;
        pos++;
    }
}

template <bool FILL, class Sink>
__device__ __forceinline__ void walk_bit_rows(const BitRows& B, const Sink& S) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * kBitRowsBlock + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * kBitRowsBlock) >> 6;
    const uint32_t W = B.W;
    if (W <= 64) {
        const uint32_t Wp = 1u << B.lg, R = 64u >> B.lg;
        const uint32_t seg = lane >> B.lg, j = lane & (Wp - 1);
        const uint64_t n_groups = (B.n_rows + R - 1) / R;
        const uint32_t mask = j + 1 == W ? B.tail : 0xFFFFFFFFu;
        for (uint64_t g = wave * kBitRowsUnroll; g < n_groups; g += n_waves * kBitRowsUnroll) {
            uint32_t w[kBitRowsUnroll], key[kBitRowsUnroll];
#pragma unroll
            for (uint32_t u = 0; u < kBitRowsUnroll; u++) {
                const uint64_t row = (g + u) * R + seg;
                key[u] = row < B.n_rows ? S.key(row, j == 0) : kNoKey;
                w[u] = (j < W && key[u] != kNoKey) ? B.bitmap[row * W + j] & mask : 0u;
            }
#pragma unroll
            for (uint32_t u = 0; u < kBitRowsUnroll; u++) {
                if (g + u >= n_groups) break;                       // (the same in every lane)
                const uint64_t row = (g + u) * R + seg;
                const uint32_t c = (uint32_t)__builtin_popcount(w[u]);
                uint32_t v = c;
                if (!FILL) {
                    for (uint32_t s = 1; s < Wp; s <<= 1) v += __shfl_xor(v, (int)s, 64);
                    if (j == 0 && row < B.n_rows) S.count(row, v);
                } else {
                    for (uint32_t s = 1; s < Wp; s <<= 1) {
                        const uint32_t o = __shfl_up(v, s, 64);
                        if (j >= s) v += o;
                    }
                    if (w[u]) emit_bits(S, key[u], w[u], j, S.base(row) + (v - c));   // (w != 0: j < W, row < n_rows, a key)
                }
            }
        }
    } else {
        for (uint64_t row = wave; row < B.n_rows; row += n_waves) {
            const uint32_t key = S.key(row, lane == 0);             // (the same in every lane)
            if (key == kNoKey) {
                if (!FILL && lane == 0) S.count(row, 0);
                continue;
            }
            const uint32_t* r = B.bitmap + row * W;
            uint64_t carry = FILL ? S.base(row) : 0;
            uint32_t acc = 0;
            for (uint32_t k = 0; k < W; k += 64) {
                const uint32_t j = k + lane;
                const uint32_t w = j < W ? r[j] & (j + 1 == W ? B.tail : 0xFFFFFFFFu) : 0u;
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
                    if (w) emit_bits(S, key, w, j, carry + (v - c));
                    carry += __shfl(v, 63, 64);
                }
            }
            if (!FILL) {
#pragma unroll
                for (uint32_t s = 1; s < 64; s <<= 1) acc += __shfl_xor(acc, (int)s, 64);
                if (lane == 0) S.count(row, acc);
            }
        }
    }
}

// ---- join_bit_rows: an arbitrary value per word, joined over the row ----------------------------------------------------------
// The same walk for a row that is not counted but compared (gft_select.hip: with `want`; gft_route.hip: with every mask).  One
// group of 64 / W' rows in flight, no tail mask (the sinks' column words are cut to n_cols), W == 0 is the caller's.  The sink:
//   Value, Col                  what is joined; what a lane knows about its column
//   Value identity()            the row of no words, and what an idle lane holds
//   Col column(j)               word j's column context, j < W: asked once in front of the loop for W <= 64 (the stores of finish
//                               keep the compiler from hoisting it on its own), per step above that
//   Value word(w, col)          what word w of a row says
//   Value join(a, b)
//   Value exchange(v, s)        v of the lane s away (xor)
//   void finish(row, v)         the finished row, in one lane
template <class Sink>
__device__ __forceinline__ void join_bit_rows(const BitRows& B, const Sink& S) {
    using Value = typename Sink::Value;
    const WaveId id(kBitRowsBlock);
    const uint32_t W = B.W;
    if (W <= 64) {
        const uint32_t Wp = 1u << B.lg, R = 64u >> B.lg;
        const uint32_t seg = id.lane >> B.lg, j = id.lane & (Wp - 1);
        typename Sink::Col col{};
        if (j < W) col = S.column(j);
        const uint64_t n_groups = (B.n_rows + R - 1) / R;
        for (uint64_t g = id.wave; g < n_groups; g += id.n_waves) {
            const uint64_t row = g * R + seg;
            Value v = (j < W && row < B.n_rows) ? S.word(B.bitmap[row * W + j], col) : S.identity();
            for (uint32_t s = 1; s < Wp; s <<= 1) v = S.join(v, S.exchange(v, s));
            if (j == 0 && row < B.n_rows) S.finish(row, v);
        }
    } else {
        for (uint64_t row = id.wave; row < B.n_rows; row += id.n_waves) {
            const uint32_t* r = B.bitmap + row * W;
            Value v = S.identity();                                 // (the carry from step to step)
            for (uint32_t k = 0; k < W; k += 64) {
                const uint32_t j = k + id.lane;
                if (j < W) v = S.join(v, S.word(r[j], S.column(j)));
            }
            for (uint32_t s = 1; s < 64; s <<= 1) v = S.join(v, S.exchange(v, s));
            if (id.lane == 0) S.finish(row, v);
        }
    }
}

// blocks of kBitRowsBlock threads for a kernel around join_bit_rows; flat: it has no words to walk and takes a thread a row
inline unsigned join_rows_grid(const BitRows& B, bool flat, unsigned n_cus) {
    const uint64_t waves = flat ? (B.n_rows + 63) / 64 : B.W <= 64 ? (B.n_rows + (64u >> B.lg) - 1) / (64u >> B.lg) : B.n_rows;
    return wave_grid(waves, kBitRowsBlock, n_cus);
}

}  // namespace gft
