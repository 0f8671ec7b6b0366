// gft_rank_piece.hpp -- what the ranking calls decide, in ONE place: gft_score_docs_device, gft_top_docs_device and
// gft_gather_docs_device.  gft_rank.hip compiles it for the device, rank_host.cpp for the host walks behind gft_debug_score_docs,
// gft_debug_top_docs and gft_debug_gather_docs, the check program tools/rank_check.cpp through that file.
//
// The score walk is the term statistics' (gft_stats_piece.hpp): workgroup w of G owns the documents [stats_cut(w), stats_cut(w + 1)),
// walks them in steps of whole documents (kStatsStepDocs documents, kStatsStep entries at most) and gives a document of kStatsLarge
// entries or more a step of its own.  The sink differs: a step keeps one 64-bit sum per document in LDS, a lane adds its entry's
// weight to its document's sum, and the step's sums go out by plain stores -- a document has one owner.  In the distinct mode an
// entry that is not the first of its (document, term) pair adds nothing: the step's set, the large path's bitset, as the docs
// counter of the statistics.  The weights lie in LDS while n_terms <= kRankWeightLdsTerms.
//
// The top call selects the k-th largest score T by radix select over the 64-bit key, kRankDigitBits bits a pass from the digit that
// holds the maximum's top bit down: a histogram of the digit over the keys that share the prefix found so far, then a pick by one
// wave -- lane l owns the bins rank_pick_bin(l, 0 .. kRankPickBins - 1), largest digit first.  The place pass then keeps score > T and
// the first r = k - c documents in index order with score == T (c: the scores above T), a tile of kRankPlaceTile documents a
// workgroup, ranks by ballot and the tiles' prefix sums.  One workgroup sorts the candidates by rank_before.
#pragma once
#include <stdint.h>

#include "gft_stats_piece.hpp"

namespace gft {

constexpr uint32_t kRankBlock = kStatsBlock;              // lanes of a workgroup of the score, histogram and place passes
constexpr uint32_t kRankTrips = kStatsStep / kRankBlock;  // entries of a step a lane takes
constexpr uint32_t kRankWeightLdsTerms = 8192;            // n_terms up to which the weights lie in LDS (32 KB)
constexpr uint32_t kRankDigitBits = 8;                    // bits of the key a select pass decides
constexpr uint32_t kRankBins = 1u << kRankDigitBits;
constexpr uint32_t kRankPickBins = kRankBins / 64;        // bins a lane of the pick's wave owns
constexpr uint32_t kRankMaxPasses = 64 / kRankDigitBits;
constexpr uint32_t kRankHistDocs = 4096;                  // documents a workgroup of the histogram pass takes at least
constexpr uint32_t kRankPlaceTrips = 4;
constexpr uint32_t kRankPlaceTile = kRankBlock * kRankPlaceTrips;   // documents of a place workgroup
constexpr uint32_t kRankPlaceRows = kRankPlaceTrips * (kRankBlock / 64);   // (trip, wave) pairs of a tile: 64 documents each
constexpr uint32_t kRankMaxK = 4096;                      // candidates one workgroup sorts in LDS (16 bytes each)
constexpr uint32_t kRankSortBlock = 1024;                 // lanes of the sort's workgroup
constexpr uint32_t kRankGatherBlock = 256;                // lanes of a workgroup of the gather's place pass

// the control block: the check pass's two flags (the statistics' words), the largest score, the select's state (the prefix is the
// threshold T after the last pass), the documents listed; the gather's flag and the text's range doc_off[0], doc_off[n_docs]
constexpr uint32_t kRankCtlMax = 2, kRankCtlPrefix = 3, kRankCtlKrem = 4, kRankCtlNTop = 5, kRankCtlBadIdx = 6, kRankCtlLo = 7, kRankCtlHi = 8,
                   kRankCtlWords = 10;
static_assert(kStatsCtlOffs == 0 && kStatsCtlTerms == 1, "the check pass is the statistics'");
static_assert(kRankBins % 64 == 0 && 64 % kRankDigitBits == 0, "whole lanes, whole passes");
static_assert((kRankMaxK & (kRankMaxK - 1)) == 0 && kRankMaxK % kRankSortBlock == 0, "the sort's network");

GFT_HD inline bool rank_weights_in_lds(uint32_t n_terms) { return n_terms <= kRankWeightLdsTerms; }

// ---- the select --------------------------------------------------------------------------------------------------------------
// digit passes for a largest score of mx: the digits above its top bit are 0 in every key
GFT_HD inline uint32_t rank_passes(uint64_t mx) {
    uint32_t p = 0;
    while (mx) { p++; mx >>= kRankDigitBits; }
    return p;
}
GFT_HD inline uint32_t rank_digit(uint64_t key, uint32_t shift) { return (uint32_t)(key >> shift) & (kRankBins - 1); }
// the key agrees with the prefix in every bit above the digit at `shift`
GFT_HD inline bool rank_in_prefix(uint64_t key, uint64_t prefix, uint32_t shift) {
    const uint32_t hi = shift + kRankDigitBits;
    return hi >= 64 || (key >> hi) == (prefix >> hi);
}
// bin j of lane l of the pick's wave: lane 0 owns the largest digits, j = 0 the largest of them
GFT_HD inline uint32_t rank_pick_bin(uint32_t lane, uint32_t j) { return kRankBins - 1 - (lane * kRankPickBins + j); }
// the lane whose bins hold the krem-th largest key (krem >= 1): `above` keys lie in bins of the lanes in front of it, `mine` in
// its own bins (cnt[j] in bin rank_pick_bin(lane, j)), above < krem <= above + mine.  Returns the digit; krem becomes the rank
// among the keys of that digit
GFT_HD inline uint32_t rank_pick_in_lane(const uint64_t (&cnt)[kRankPickBins], uint32_t lane, uint64_t above, uint64_t& krem) {
    uint64_t k = krem - above;
    uint32_t j = 0;
    while (j + 1 < kRankPickBins && k > cnt[j]) { k -= cnt[j]; j++; }
    krem = k;
    return rank_pick_bin(lane, j);
}

// ---- the place pass ----------------------------------------------------------------------------------------------------------
// what a score is to the threshold T: 2 above it, 1 equal to it (a score of 0 is never listed), 0 dropped
GFT_HD inline uint32_t rank_class(uint64_t score, uint64_t T) { return score > T ? 2u : (score == T && T) ? 1u : 0u; }
// the equals that are listed: c scores above T, eq equal to it
GFT_HD inline uint64_t rank_equals_kept(uint64_t k, uint64_t c, uint64_t eq) { return c >= k ? 0 : (eq < k - c ? eq : k - c); }
// document i of tile t in the order the tile's lanes take them: trip major, lane minor -- index order
GFT_HD inline uint64_t rank_place_doc(uint64_t tile, uint32_t trip, uint32_t tid) { return tile * kRankPlaceTile + (uint64_t)trip * kRankBlock + tid; }
GFT_HD inline uint32_t rank_place_row(uint32_t trip, uint32_t wave) { return trip * (kRankBlock / 64) + wave; }

// ---- the sort ----------------------------------------------------------------------------------------------------------------
// the total order: larger score first, among equal scores the smaller document index first
GFT_HD inline bool rank_before(uint64_t sa, uint64_t ia, uint64_t sb, uint64_t ib) { return sa > sb || (sa == sb && ia < ib); }
// the network's size for n candidates: a power of two, 2 at least; the slots behind n hold (0, UINT64_MAX), which sorts last
GFT_HD inline uint32_t rank_sort_size(uint32_t n) {
    uint32_t s = 2;
    while (s < n) s <<= 1;
    return s;
}
// one compare-exchange of the bitonic network: slot i in the stage (kk, j) meets slot i ^ j; false when i is the upper of the pair
// (the lower one acts); up: the pair sorts towards rank_before
GFT_HD inline bool rank_sort_pair(uint32_t i, uint32_t j, uint32_t kk, uint32_t& other, bool& up) {
    other = i ^ j;
    up = (i & kk) == 0;
    return other > i;
}

// ---- the gather --------------------------------------------------------------------------------------------------------------
// list entry v is document v - idx_base: true when that is one of the n_docs (an index below the base wraps and fails)
GFT_HD inline bool rank_gather_doc(uint64_t v, uint64_t idx_base, uint64_t n_docs, uint64_t& d) {
    d = v - idx_base;
    return v >= idx_base && d < n_docs;
}

}  // namespace gft
