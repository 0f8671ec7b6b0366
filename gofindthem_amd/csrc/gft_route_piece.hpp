// gft_route_piece.hpp -- documents routed to per-bucket runs of one blob (gft_route_docs_device): what a word of a row says about the
// buckets, what a document's member word is, and where an entry of a tile lands, shared by the kernels (gft_route.hip) and the
// host walk (route_host.cpp).
//
// The route is a stable counting sort of (document, bucket) entries.  A document's member word has bit b set when the document
// has an entry in bucket b (b < n_buckets: a mask it hits; b == n_buckets: the rest bucket).  The documents are cut into tiles of
// kRouteTileDocs = 64, a wave each and a lane a document: the entries of bucket b in a tile are the set bits of one ballot, their
// count its popcount, and the rank of a lane's entry the popcount of the ballot below the lane.  The counts lie bucket-major,
// cnt[b * n_tiles + tile], so ONE exclusive prefix sum over B * n_tiles entries gives every (bucket, tile) its first rank, the
// bucket borders (the entries at b * n_tiles) and the number of entries m (the last one).
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

constexpr uint32_t kRouteTileDocs = 64;                    // documents per counting tile: a wave, a lane a document

GFT_HD inline uint64_t route_tiles(uint64_t n_docs) { return (n_docs + kRouteTileDocs - 1) / kRouteTileDocs; }
GFT_HD inline uint64_t route_cell(uint32_t b, uint64_t n_tiles, uint64_t tile) { return (uint64_t)b * n_tiles + tile; }

// ---- the mark pass ---------------------------------------------------------------------------------------------------------
// one word of a row against the same word of bucket k's mask (already cut to n_cols): bit k when they meet
GFT_HD inline uint64_t route_word_bit(uint32_t w, uint32_t mask_word, uint32_t k) { return (w & mask_word) ? 1ull << k : 0ull; }
// the FIRST cut: the lowest set bit alone
GFT_HD inline uint64_t route_first(uint64_t hits) { return hits & (~hits + 1); }
// A document's member word from the buckets its row hits (bits below n_buckets): the mode's cut, then the rest bucket -- bit
// n_buckets, when the flag is on and nothing hit -- and `also`, which sends the document to the rest bucket and nowhere else.
GFT_HD inline uint64_t route_member(uint64_t hits, uint32_t n_buckets, uint32_t mode, uint32_t rest, uint32_t also) {
    if (mode == GFT_ROUTE_FIRST) hits = route_first(hits);
    if (rest && (also || !hits)) hits = 1ull << n_buckets;
    return hits;
}

// ---- the count and place passes --------------------------------------------------------------------------------------------
GFT_HD inline uint64_t route_lanes_below(uint32_t lane) { return lane ? ~0ull >> (64 - lane) : 0ull; }
GFT_HD inline uint32_t route_popcount(uint64_t v) { return (uint32_t)__builtin_popcountll(v); }
// the rank of lane's entry in a bucket: the (bucket, tile) base plus the entries of the lanes below
GFT_HD inline uint64_t route_rank(uint64_t base, uint64_t ballot, uint32_t lane) { return base + route_popcount(ballot & route_lanes_below(lane)); }
// the bytes a document adds to the output: its length once per entry
GFT_HD inline uint64_t route_doc_bytes(uint32_t len, uint64_t member) { return (uint64_t)len * route_popcount(member); }

}  // namespace gft
