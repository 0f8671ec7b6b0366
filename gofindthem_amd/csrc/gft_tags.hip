// gft_tags.hip -- leaf hit bitmap of a record batch -> per-record lists of (field, expression): the batch form of TagObject's
// map (group/finder/finder.go:87-110, internal.go:9-38), gfx950 / wave64.  The tag-side counterpart of gft_compact.hip.
//
//   hit rows [n_leaves][W] (W = ceil(n_exprs / 32)), leaf_field [n_leaves], rec_off [n_records + 1], valid [ceil(F / 32)]  ->
//   row_off [n_records + 1] u64, ent_field / ent_expr / ent_tag [total] u32: leaves in record order, expressions ascending
//   inside a leaf
//
//   k_tags<false>  popcount per leaf row, the row taken as zero when the leaf's field is invalid or outside the schema
//                                                                                   -> cnt [n_leaves] u32
//   (k_scan_partials / k_scan_spine / k_scan_final of gft_kernels.hip: cnt -> leaf_ent_off [n_leaves + 1])
//   k_tags<true>   row_off[r] = leaf_ent_off[rec_off[r]], every word once with a plain store; then the exclusive prefix of
//                  the word popcounts inside a row, and every lane writes the set bits of its word, lowest first, at
//                  leaf_ent_off[leaf] + prefix
//
// Both passes read the bitmap as k_compact does, the lanes of a wave on consecutive words.  W <= 64: a wave takes 64 / W'
// leaves at once (W' = W rounded up to a power of two; a leaf is a segment of W' lanes, the lanes W..W'-1 of a segment idle)
// and reduces / scans per segment with shuffles, kTagsUnroll groups in flight.  W > 64: a wave walks one row in steps of 64
// words with a carry.  W is a run-time value.  Nothing is stored at or past `cap` entries; bits at and above n_exprs in a
// row's last word are masked.  The passes also validate what they read: a field index outside the schema sets flags[0] (count
// pass), record offsets that descend, leave [0, n_leaves] or do not end at n_leaves set flags[1] (fill pass) -- plain stores
// of 1; such leaves count nothing and such offsets are never used as an index.  Memory bound: two reads of the bitmap plus
// the output.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gft_tags.hpp"

namespace gft {

namespace {

constexpr uint32_t kTagsBlock = 256;     // 4 waves
constexpr uint32_t kTagsUnroll = 4;      // leaf groups a wave has in flight (W <= 64): the loads of four before the first use
constexpr uint32_t kNoField = 0xFFFFFFFFu;

// the field of a leaf when the leaf contributes, kNoField otherwise
__device__ __forceinline__ uint32_t contributing_field(const TagParams& P, uint64_t leaf) {
    if (leaf >= P.n_leaves) return kNoField;
    const uint32_t f = P.leaf_field[leaf];
    if (f >= P.n_fields) return kNoField;
    return (P.valid[f >> 5] >> (f & 31) & 1u) ? f : kNoField;
}

// the set bits of word j of a leaf's row, lowest first, to positions pos, pos + 1, ...
__device__ __forceinline__ void write_entries(const TagParams& P, uint32_t w, uint32_t j, uint32_t field, uint64_t pos) {
    while (w) {
        const uint32_t x = j * 32u + (uint32_t)__builtin_ctz(w);
        w &= w - 1;
        if (pos < P.cap) {
            P.ent_expr[pos] = x;
            P.ent_field[pos] = field;
            if (P.ent_tag) P.ent_tag[pos] = P.expr_tag[x];
        }
        pos++;
    }
}

template <bool FILL>
__global__ void __launch_bounds__(kTagsBlock) k_tags(const TagParams P) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t tid = (uint64_t)blockIdx.x * kTagsBlock + threadIdx.x;
    const uint64_t n_threads = (uint64_t)gridDim.x * kTagsBlock;
    const uint64_t wave = tid >> 6, n_waves = n_threads >> 6;
    const uint32_t W = P.W;
    if (FILL) {
        // the records' offsets into the entries, gathered through rec_off once that is known to be an index
        for (uint64_t r = tid; r <= P.n_records; r += n_threads) {
            const uint64_t o = P.rec_off[r];
            const bool last = r == P.n_records;
            if (o > P.n_leaves || (last ? o != P.n_leaves : P.rec_off[r + 1] < o)) P.flags[1] = 1;
            P.row_off[r] = o <= P.n_leaves ? P.leaf_ent_off[o] : 0;
        }
        if (!P.cap || !W) return;
    } else if (!W) {                                 // a finder without expressions: nothing to count, the fields are still checked
        for (uint64_t l = tid; l < P.n_leaves; l += n_threads) {
            if (P.leaf_field[l] >= P.n_fields) P.flags[0] = 1;
            P.cnt[l] = 0;
        }
        return;
    }
    if (W <= 64) {
        const uint32_t Wp = 1u << P.lg, R = 64u >> P.lg;
        const uint32_t seg = lane >> P.lg, j = lane & (Wp - 1);
        const uint64_t n_groups = (P.n_leaves + R - 1) / R;
        const uint32_t mask = j + 1 == W ? P.tail : 0xFFFFFFFFu;
        for (uint64_t g = wave * kTagsUnroll; g < n_groups; g += n_waves * kTagsUnroll) {
            uint32_t w[kTagsUnroll], f[kTagsUnroll];
#pragma unroll
            for (uint32_t u = 0; u < kTagsUnroll; u++) {
                const uint64_t leaf = (g + u) * R + seg;
                f[u] = contributing_field(P, leaf);
                if (!FILL && j == 0 && leaf < P.n_leaves && P.leaf_field[leaf] >= P.n_fields) P.flags[0] = 1;
                w[u] = (j < W && f[u] != kNoField) ? P.bitmap[leaf * W + j] & mask : 0u;
            }
#pragma unroll
            for (uint32_t u = 0; u < kTagsUnroll; u++) {
                if (g + u >= n_groups) break;                       // (the same in every lane)
                const uint64_t leaf = (g + u) * R + seg;
                const uint32_t c = (uint32_t)__builtin_popcount(w[u]);
                uint32_t v = c;
                if (!FILL) {
                    for (uint32_t s = 1; s < Wp; s <<= 1) v += __shfl_xor(v, (int)s, 64);
                    if (j == 0 && leaf < P.n_leaves) P.cnt[leaf] = v;
                } else {
                    for (uint32_t s = 1; s < Wp; s <<= 1) {
                        const uint32_t o = __shfl_up(v, s, 64);
                        if (j >= s) v += o;
                    }
                    if (w[u]) write_entries(P, w[u], j, f[u], P.leaf_ent_off[leaf] + (v - c));   // (w != 0: j < W, leaf < n_leaves, a valid field)
                }
            }
        }
    } else {
        for (uint64_t leaf = wave; leaf < P.n_leaves; leaf += n_waves) {
            const uint32_t f = contributing_field(P, leaf);         // (the same in every lane)
            if (f == kNoField) {
                if (!FILL && lane == 0) {
                    if (P.leaf_field[leaf] >= P.n_fields) P.flags[0] = 1;
                    P.cnt[leaf] = 0;
                }
                continue;
            }
            const uint32_t* r = P.bitmap + leaf * W;
            uint64_t carry = FILL ? P.leaf_ent_off[leaf] : 0;
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
                    if (w) write_entries(P, w, j, f, carry + (v - c));
                    carry += __shfl(v, 63, 64);
                }
            }
            if (!FILL) {
#pragma unroll
                for (uint32_t s = 1; s < 64; s <<= 1) acc += __shfl_xor(acc, (int)s, 64);
                if (lane == 0) P.cnt[leaf] = acc;
            }
        }
    }
}

unsigned tags_grid(const TagParams& P, uint64_t n_records, unsigned n_cus) {
    // waves that have work: a group of 64 / W' leaves per wave and trip (W <= 64), a leaf per wave otherwise; W == 0: a thread a leaf
    uint64_t blocks;
    if (!P.W) {
        blocks = (P.n_leaves + kTagsBlock - 1) / kTagsBlock;
    } else {
        const uint64_t items = P.W <= 64 ? (P.n_leaves + (64u >> P.lg) - 1) / (64u >> P.lg) : P.n_leaves;
        const uint64_t per_wave = P.W <= 64 ? kTagsUnroll : 1;
        blocks = (items + per_wave * (kTagsBlock / 64) - 1) / (per_wave * (kTagsBlock / 64));
    }
    blocks = std::max<uint64_t>(blocks, (n_records + kTagsBlock) / kTagsBlock);       // (the fill pass: a thread per row_off word)
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)std::max(n_cus, 1u) * 8));   // 32 waves per CU
}

}  // namespace

TagParams tag_params(const uint32_t* d_bitmap, uint32_t n_exprs, const uint32_t* d_leaf_field, const uint32_t* d_valid, uint32_t n_fields,
                     uint64_t n_leaves, uint32_t* d_flags) {
    TagParams P{};
    P.bitmap = d_bitmap;
    P.leaf_field = d_leaf_field;
    P.valid = d_valid;
    P.n_leaves = n_leaves;
    P.n_fields = n_fields;
    P.W = (n_exprs + 31) / 32;
    while ((1u << P.lg) < P.W && P.lg < 6) P.lg++;
    P.tail = (n_exprs & 31) ? (1u << (n_exprs & 31)) - 1 : 0xFFFFFFFFu;
    P.flags = d_flags;
    return P;
}

hipError_t launch_tags_count(const TagParams& P, unsigned n_cus, hipStream_t st) {
    if (!P.n_leaves) return hipSuccess;
    k_tags<false><<<dim3(tags_grid(P, 0, n_cus)), dim3(kTagsBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_tags_fill(const TagParams& P, unsigned n_cus, hipStream_t st) {
    k_tags<true><<<dim3(tags_grid(P, P.n_records, n_cus)), dim3(kTagsBlock), 0, st>>>(P);
    return hipGetLastError();
}

}  // namespace gft
