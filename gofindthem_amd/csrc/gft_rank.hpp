// gft_rank.hpp -- a score per document, the k best documents of a score array and documents gathered by an index list
// (gft_rank.hip): the launchers, and the same walks on the host (rank_host.cpp).
#pragma once
#include <stdint.h>

#include "../../include/gft.h"
#include "gft_overlap.hpp"
#include "gft_rank_piece.hpp"
#include "gft_select_piece.hpp"

namespace gft {

// gft_score_docs_device's contract on host pointers: the check, then the walk workgroup by workgroup, step by step and lane by
// lane through gft_rank_piece.hpp (the set and the bitset included).  Returns a gft_status; a refusal writes nothing.
int score_docs_host(const uint64_t* off, const uint32_t* term, uint64_t n_docs, uint32_t n_terms, const uint32_t* weights, uint32_t flags,
                    uint64_t* score, uint64_t* max_score);
// gft_top_docs_device's contract on host pointers: the maximum, the select pass by pass with the pick lane by lane, the place pass
// tile by tile, the sort's network stage by stage
int top_docs_host(const uint64_t* score, uint64_t n_docs, uint32_t k, uint64_t doc_base, uint64_t* top_idx, uint64_t* top_score, uint64_t* n_top);
// gft_gather_docs_device's contract on host pointers: the place pass, the prefix sum, the select's copy pass tile by tile
int gather_docs_host(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* idx, uint64_t m, uint64_t idx_base, uint8_t* out,
                     uint64_t cap_bytes, uint64_t* out_off, uint64_t* total_bytes);

// the scores overlap the list (its entries are [e0, e0 + n) of term)
inline bool score_buffers_overlap(const uint64_t* off, uint64_t n_docs, const uint32_t* term, uint64_t e0, uint64_t n, const uint64_t* score) {
    const ByteRange outs[] = {{score, n_docs * 8}};
    const ByteRange ins[] = {{off, (n_docs + 1) * 8}, {term ? term + e0 : nullptr, n * 4}};
    return outputs_overlap(outs, ins);
}
// a top array overlaps the scores or the other one
inline bool top_buffers_overlap(const uint64_t* score, uint64_t n_docs, uint32_t k, const uint64_t* top_idx, const uint64_t* top_score) {
    const ByteRange outs[] = {{top_idx, (uint64_t)k * 8}, {top_score, (uint64_t)k * 8}};
    const ByteRange ins[] = {{score, n_docs * 8}};
    return outputs_overlap(outs, ins);
}
// an output of the gather overlaps an input (the text is [lo, hi) of the blob) or the other output
inline bool gather_buffers_overlap(const uint8_t* text, uint64_t lo, uint64_t hi, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* idx,
                                   uint64_t m, const uint8_t* out, uint64_t cap_bytes, const uint64_t* out_off) {
    const ByteRange outs[] = {{out, cap_bytes}, {out_off, (m + 1) * 8}};
    const ByteRange ins[] = {{text ? text + lo : nullptr, hi > lo ? hi - lo : 0}, {doc_off, (n_docs + 1) * 8}, {idx, m * 8}};
    return outputs_overlap(outs, ins);
}

}  // namespace gft

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace gft {

// Work buffers of the score call: kRankCtlWords * 8 bytes of control block, n_terms * 4 bytes of weights; in the distinct mode with
// n_terms > kStatsBitsetLdsTerms a bitset row of ceil(n_terms / 32) * 4 bytes per workgroup.  Nothing per entry or document.
struct ScoreParams {
    const uint64_t* off;           // [n_docs + 1]
    const uint32_t* term;
    uint64_t n_docs, e0, n;        // the entries are [e0, e0 + n)
    uint32_t n_terms, distinct;
    const uint32_t* weights;       // [n_terms] on the device; NULL: every term 1
    uint64_t* score;               // [n_docs]
    uint64_t* ctl;                 // [kRankCtlWords]
    uint32_t* rows;                // the workgroups' bitset rows (NULL: the bitset is in LDS, or the mode has none)
    uint32_t grid;
};

// Work buffers of the top call: the control block, kRankMaxPasses * kRankBins * 8 bytes of histograms, two 32-bit counts and two
// 64-bit prefix sums per tile of kRankPlaceTile documents (24 / kRankPlaceTile bytes per document) with the prefix sum's partials,
// 16 bytes per candidate (k of them at most).
struct TopParams {
    const uint64_t* score;         // [n_docs]
    uint64_t n_docs, n_tiles;
    uint32_t k, shift;             // shift: the digit of this select pass
    uint64_t doc_base;
    uint64_t* ctl;                 // [kRankCtlWords]
    uint64_t* hist;                // [kRankMaxPasses][kRankBins]; the pass at `shift` uses row shift / kRankDigitBits
    uint32_t* tile_gt;             // [n_tiles] scores above T, equal to T
    uint32_t* tile_eq;
    const uint64_t* gt_pos;        // [n_tiles + 1] their exclusive prefix sums
    const uint64_t* eq_pos;
    uint64_t* cand_score;          // [k]
    uint64_t* cand_idx;
    uint64_t* top_idx;             // [k] the caller's
    uint64_t* top_score;
};

struct GatherParams {
    const uint64_t* doc_off;       // [n_docs + 1]
    uint64_t n_docs;
    const uint64_t* idx;           // [m]
    uint64_t m, idx_base;
    uint32_t* len;                 // [m]
    uint64_t* c_src;               // [m]
    uint64_t* ctl;
};

hipError_t launch_score_docs(const ScoreParams& P, hipStream_t st);
hipError_t launch_top_max(const TopParams& P, unsigned n_cus, hipStream_t st);
hipError_t launch_top_hist(const TopParams& P, unsigned n_cus, hipStream_t st);
hipError_t launch_top_pick(const TopParams& P, hipStream_t st);
hipError_t launch_top_count(const TopParams& P, hipStream_t st);
hipError_t launch_top_place(const TopParams& P, hipStream_t st);
hipError_t launch_top_sort(const TopParams& P, hipStream_t st);
hipError_t launch_gather_place(const GatherParams& P, unsigned n_cus, hipStream_t st);

}  // namespace gft
#endif
