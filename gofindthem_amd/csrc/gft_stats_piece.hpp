// gft_stats_piece.hpp -- what the term histogram and the column count decide, in ONE place: the borders of the walk and the
// functions that say which workgroup owns a document, where a step ends, which path a document takes and which slot a key
// hashes to.  gft_stats.hip compiles it for the device, stats_host.cpp for the host walk behind gft_debug_term_stats, the check
// program tools/term_stats_check.cpp through that file.
//
// The walk.  The list's weight is its entries plus its documents (a document costs an offset, an entry a term).  Workgroup w of
// G owns the documents [stats_cut(w), stats_cut(w + 1)): cut at document borders, near-equal weight.  It walks them in STEPS of
// whole documents: at most kStatsStepDocs documents holding at most kStatsStep entries together.  Inside a step a lane takes an
// entry, finds its document in the step's offsets (LDS) and asks the step's SET -- kStatsSetSlots keys (document in step + 1,
// term), open addressing, compare-and-swap -- whether it is the first of its pair.  A document of kStatsLarge entries or more is
// a step of its own, taken kStatsStep entries at a time, with a BITSET of n_terms bits and test-and-set instead of the set: in
// the set's LDS while n_terms <= kStatsBitsetLdsTerms, in a row of the workgroup's in global memory above that.  Either way an
// entry then is (term, 1, first of its pair ? 1 : 0, document) and goes to the workgroup's CACHE: kStatsCacheSlots slots of
// (term, occ, docs, first), direct-mapped.  A slot that holds another term is evicted to the global counters once per step and
// slot, by one of the lanes that met it; a lane that still finds another term there afterwards adds to the global counters
// itself.  The cache is flushed when the workgroup's range ends (and before a 32-bit counter in it could wrap).
#pragma once
#include <stdint.h>

#ifndef GFT_HD
#if defined(__HIPCC__)
#define GFT_HD __host__ __device__
#else
#define GFT_HD
#endif
#endif

namespace gft {

constexpr uint32_t kStatsBlock = 256;                     // lanes of a workgroup
constexpr uint32_t kStatsStep = 1024;                     // entries of a step at most
constexpr uint32_t kStatsStepDocs = 1024;                 // documents of a step at most
constexpr uint32_t kStatsLarge = kStatsStep + 1;          // entries at which a document takes the large path
constexpr uint32_t kStatsSetSlots = 2048;                 // keys of the step's set (8 bytes each), twice a step's entries
constexpr uint32_t kStatsCacheSlots = 1024;               // slots of the workgroup's cache
constexpr uint32_t kStatsBitsetLdsTerms = kStatsSetSlots * 64;   // n_terms up to which the bitset lies in LDS (the set's bytes)
constexpr uint32_t kStatsRangeWeight = 4 * kStatsStep;    // weight a workgroup owns at least (but for the last)
constexpr uint32_t kStatsFlushEntries = 0x7FFFFFFFu;      // entries a workgroup takes between two flushes of its cache at most
constexpr uint32_t kStatsNoTerm = 0xFFFFFFFFu;            // an empty cache slot (a term id is < n_terms <= 2^32 - 1)
constexpr uint32_t kStatsColRows = 2048;                  // rows a workgroup of the column count owns
constexpr uint32_t kStatsCtlOffs = 0, kStatsCtlTerms = 1, kStatsCtlWords = 2;   // the check pass's flag words

static_assert(kStatsSetSlots >= 2 * kStatsStep && (kStatsSetSlots & (kStatsSetSlots - 1)) == 0, "the set never fills");
static_assert((kStatsCacheSlots & (kStatsCacheSlots - 1)) == 0, "slots by mask");
static_assert(kStatsStep % kStatsBlock == 0 && kStatsColRows % kStatsBlock == 0, "whole trips");

// workgroups of the count pass for n entries in n_docs documents on a device that holds `resident` of them at a time
GFT_HD inline uint64_t stats_grid(uint64_t n, uint64_t n_docs, uint64_t resident) {
    const uint64_t g = (n + n_docs + kStatsRangeWeight - 1) / kStatsRangeWeight;
    return g < 1 ? 1 : g > resident ? resident : g;
}

// the first document of workgroup w of G: 0 for w = 0, n_docs for w = G, else the first document with w / G of the weight in
// front of it.  A document is never split; cuts ascend with w.  off: n_docs + 1 ascending offsets
GFT_HD inline uint64_t stats_cut(const uint64_t* off, uint64_t n_docs, uint64_t w, uint64_t G) {
    if (w == 0) return 0;
    if (w >= G) return n_docs;
    const uint64_t e0 = off[0], total = off[n_docs] - e0 + n_docs;
    const uint64_t target = (total / G) * w + (total % G) * w / G;
    uint64_t lo = 0, hi = n_docs;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (off[mid] - e0 + mid < target) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// a step's offsets as the workgroup keeps them: entries in front of document d0 + k, relative to d0's first, capped
GFT_HD inline uint32_t stats_rel(uint64_t off_k, uint64_t off_0) {
    const uint64_t v = off_k - off_0;
    return v > kStatsStep ? kStatsStep + 1 : (uint32_t)v;
}

// the documents of the step that begins at d0: the largest k <= tries with rel[k] <= kStatsStep; 0: d0 takes the large path
// (rel[0] = 0, rel ascends)
template <class Rel>
GFT_HD inline uint32_t stats_step_docs(const Rel& rel, uint32_t tries) {
    uint32_t lo = 0, hi = tries;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) / 2;
        if (rel[mid] <= kStatsStep) lo = mid; else hi = mid - 1;
    }
    return lo;
}

GFT_HD inline bool stats_doc_large(uint64_t entries) { return entries >= kStatsLarge; }

// the document in the step (of nd documents) that holds the step's entry i: the last k with rel[k] <= i
template <class Rel>
GFT_HD inline uint32_t stats_find_doc(const Rel& rel, uint32_t nd, uint32_t i) {
    uint32_t lo = 0, hi = nd - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) / 2;
        if (rel[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

GFT_HD inline uint64_t stats_set_key(uint32_t doc_in_step, uint32_t term) { return (uint64_t)(doc_in_step + 1) << 32 | term; }
GFT_HD inline uint32_t stats_set_slot(uint32_t doc_in_step, uint32_t term) { return (term + doc_in_step * 0x9E5u) & (kStatsSetSlots - 1); }
GFT_HD inline uint32_t stats_set_next(uint32_t slot) { return (slot + 1) & (kStatsSetSlots - 1); }
GFT_HD inline uint32_t stats_cache_slot(uint32_t term) { return term & (kStatsCacheSlots - 1); }
GFT_HD inline bool stats_bitset_in_lds(uint32_t n_terms) { return n_terms <= kStatsBitsetLdsTerms; }
GFT_HD inline uint64_t stats_bitset_words(uint32_t n_terms) { return ((uint64_t)n_terms + 31) / 32; }

// the column count: words of a row, the row a workgroup's lane counts
GFT_HD inline uint32_t stats_col_words(uint32_t n_cols) { return (n_cols + 31) / 32; }
GFT_HD inline uint32_t stats_col_mask(uint32_t n_cols, uint32_t word) {
    const uint32_t left = n_cols - word * 32;
    return left >= 32 ? 0xFFFFFFFFu : (1u << left) - 1;
}

}  // namespace gft
