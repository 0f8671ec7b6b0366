// gft_context_piece.hpp -- context lines round the documents that matched (gft_context_docs_device): what a tile of 64 documents, a
// lane of it and a carry say, shared by the kernels (gft_context.hip) and the host walk (context_host.cpp).
//
// Document d is kept when a selected h with d - after <= h <= d + before exists that no fence separates from d; a fence at f
// (d_fence[f] != 0) separates h and d when f lies in (min(h, d), max(h, d)].  Only the NEAREST selected document on either side can
// decide that: a farther one is farther, and every fence in front of the nearer lies in front of it too.  So a document needs four
// indices: the last selected and the last fence at or in front of it, the first selected at or behind it and the first fence
// behind it.  Inside its tile they are clz / ctz on the tile's two ballot words under a lane mask; outside they are the tile's
// carry: running maxima over the tiles in front, running minima over the tiles behind.  No segmented operator: the selected h in
// front counts iff h >= the last fence, the one behind iff h < the first fence.
//
// Encodings: a "last" index is stored as index + 1 with 0 for none (the identity of max), a "first" index as it is with kCtxNone
// for none (the identity of min).  Indices stay below 2^60.
#pragma once
#include <stdint.h>

#include "../../include/gft.h"

#ifndef GFT_HD
#if defined(__HIPCC__)
#define GFT_HD __host__ __device__
#else
#define GFT_HD
#endif
#endif

namespace gft {

constexpr uint32_t kCtxTile = 64;          // documents per tile: a wave, a document a lane
constexpr uint32_t kCtxCarry = 64;         // tiles per carry block: a wave, a tile a lane
constexpr uint32_t kCtxSpine = 64;         // carry blocks per trip of the spine: one wave, a block a lane
constexpr uint64_t kCtxNone = ~0ull;

GFT_HD inline uint64_t ctx_tiles(uint64_t n_docs) { return (n_docs + kCtxTile - 1) / kCtxTile; }
GFT_HD inline uint64_t ctx_blocks(uint64_t n_tiles) { return (n_tiles + kCtxCarry - 1) / kCtxCarry; }

GFT_HD inline uint64_t ctx_max(uint64_t a, uint64_t b) { return a > b ? a : b; }
GFT_HD inline uint64_t ctx_min(uint64_t a, uint64_t b) { return a < b ? a : b; }
// the highest / lowest set bit of a word that has one
GFT_HD inline uint32_t ctx_top(uint64_t w) { return 63u - (uint32_t)__builtin_clzll(w); }
GFT_HD inline uint32_t ctx_low(uint64_t w) { return (uint32_t)__builtin_ctzll(w); }

// ---- the reach pass: what a tile's word (selected, or fence; bit l = document base + l) says to the tiles round it ------------
GFT_HD inline uint64_t ctx_last(uint64_t w, uint64_t base) { return w ? base + ctx_top(w) + 1 : 0; }
GFT_HD inline uint64_t ctx_first(uint64_t w, uint64_t base) { return w ? base + ctx_low(w) : kCtxNone; }

// ---- the decide pass ---------------------------------------------------------------------------------------------------------------
// what lies outside a tile: over the tiles in front the last selected and the last fence, over the tiles behind the first of each
struct CtxCarry {
    uint64_t prev_sel, prev_fence;         // index + 1; 0: none
    uint64_t next_sel, next_fence;         // index; kCtxNone: none
};
// the nearest selected document at or in front of lane l's that no fence separates from it: index + 1; 0: none
GFT_HD inline uint64_t ctx_back(uint64_t S, uint64_t F, const CtxCarry& c, uint64_t base, uint32_t l) {
    const uint64_t m = ~0ull >> (63u - l);                          // the lanes 0 .. l
    const uint64_t h = ctx_max(ctx_last(S & m, base), c.prev_sel);
    const uint64_t f = ctx_max(ctx_last(F & m, base), c.prev_fence);
    return h >= f ? h : 0;                                          // (a fence ON h does not separate it from what follows)
}
// ... at or behind it: index; kCtxNone: none
GFT_HD inline uint64_t ctx_ahead(uint64_t S, uint64_t F, const CtxCarry& c, uint64_t base, uint32_t l) {
    const uint64_t ms = ~0ull << l;                                 // the lanes l .. 63
    const uint64_t mf = l == 63 ? 0 : ~0ull << (l + 1);             // the lanes l + 1 .. 63: a fence on d itself lies in front of d
    const uint64_t h = ctx_min(ctx_first(S & ms, base), c.next_sel);
    const uint64_t f = ctx_min(ctx_first(F & mf, base), c.next_fence);
    return h < f ? h : kCtxNone;                                    // (a fence ON h separates it from what precedes)
}
// lane l's document is kept.  The differences cannot wrap, so before and after may be 2^64 - 1
GFT_HD inline uint32_t ctx_keep(uint64_t S, uint64_t F, const CtxCarry& c, uint64_t base, uint32_t l, uint64_t before, uint64_t after) {
    const uint64_t d = base + l;
    const uint64_t hb = ctx_back(S, F, c, base, l);
    if (hb && d - (hb - 1) <= after) return 1;
    const uint64_t ha = ctx_ahead(S, F, c, base, l);
    return (ha != kCtxNone && ha - d <= before) ? 1u : 0u;
}
// the document in front of the tile (base > 0) is kept: lane 0's left neighbour, from the tile's own words and carry.  At or in
// front of it lie the carries alone; behind it the whole tile, then the carry.
GFT_HD inline uint32_t ctx_keep_left(uint64_t S, uint64_t F, const CtxCarry& c, uint64_t base, uint64_t before, uint64_t after) {
    const uint64_t d = base - 1;
    if (c.prev_sel && c.prev_sel >= c.prev_fence && d - (c.prev_sel - 1) <= after) return 1;
    const uint64_t h = ctx_min(ctx_first(S, base), c.next_sel);
    const uint64_t f = ctx_min(ctx_first(F, base), c.next_fence);
    return (h < f && h - d <= before) ? 1u : 0u;
}
// lane l's document begins a group: kept, and the first document, or its left neighbour is not kept, or a fence stands on it
GFT_HD inline uint32_t ctx_new_group(uint32_t keep, uint32_t left_kept, uint64_t d, uint32_t fence_here) {
    return (keep && (d == 0 || !left_kept || fence_here)) ? 1u : 0u;
}

}  // namespace gft
