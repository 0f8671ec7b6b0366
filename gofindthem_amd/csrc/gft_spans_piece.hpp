// gft_spans_piece.hpp -- hit spans and redaction (gft_hit_spans_device, gft_redact_spans_device): what a match, a tile of spans and
// a fill position decide, shared by the kernels (gft_spans.hip) and the host walks (spans_host.cpp).
//
// Spans.  The canonical match CSR of a scan (match_off [n_docs + 1], term, pos) is filtered: match m of document d is KEPT when
// some expression i of the witness list of its term, wit_expr[wit_off[t] .. wit_off[t + 1]) (witness_terms.hpp: ascending, every
// i < n_exprs), is wanted and true in row r(d) of the hit bitmap.  Only bits i < n_exprs are ever read, one at a time, so what a
// row's or the mask's last word holds at and above n_exprs cannot matter.  keep[m] -> exclusive prefix sum rank[m] -> span
// rank[m] = (start, len, term) of every kept match, span_off[d] = rank[match_off[d]]: a stable compaction.
//
// Fill.  From the output side: a wave owns a tile of kSpanTile spans, lane l span l of the tile.  The lanes' lengths are summed
// across the wave (exclusive prefix, 64 bits: 64 spans of up to 4 GiB - 1); the tile's virtual bytes [0, sum) are walked with
// lane l on byte l + 64 j; the span of a virtual byte is the last lane whose prefix is <= it (span_fill_lane: six reads of other
// lanes' prefixes, no memory), and the lane stores ONE byte.  The work per lane is the tile's bytes / 64 whatever the spans'
// lengths, and no byte outside a span is ever part of a store.
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

constexpr uint32_t kSpanMarkBlock = 256;   // matches a workgroup of the mark and place passes takes per step: the match tile
constexpr uint32_t kSpanTile = 64;         // spans a wave of the fill pass owns: one per lane

// ---- the mark pass ---------------------------------------------------------------------------------------------------------
// the document of match m: the d < n_docs with match_off[d] <= m < match_off[d + 1] (m < match_off[n_docs]; documents without a
// match are runs of equal offsets and are never the answer).  n_docs >= 1.
GFT_HD inline uint64_t span_doc_of(const uint64_t* match_off, uint64_t n_docs, uint64_t m) {
    uint64_t lo = 0, hi = n_docs - 1;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (match_off[mid + 1] <= m) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// a match of term t in a document whose row is `row`: 1 when an expression of t's witness list is wanted and true -- the walk
// stops at the first.  want == nullptr: every expression is wanted.
GFT_HD inline uint32_t span_match_kept(uint32_t t, const uint32_t* row, const uint32_t* want, const uint64_t* wit_off, const uint32_t* wit_expr) {
    for (uint64_t k = wit_off[t], end = wit_off[t + 1]; k < end; k++) {
        const uint32_t i = wit_expr[k];
        uint32_t w = row[i >> 5];
        if (want) w &= want[i >> 5];
        if ((w >> (i & 31)) & 1u) return 1u;
    }
    return 0u;
}

// ---- the place pass ----------------------------------------------------------------------------------------------------------
// where a match of `len` bytes reported at `pos` begins: pos is its first byte on a GFT_POS_START engine, its last on a GFT_POS_END one
GFT_HD inline uint32_t span_start_of(uint32_t pos, uint32_t len, uint32_t pos_end) { return pos_end ? pos + 1u - len : pos; }

// ---- the redaction --------------------------------------------------------------------------------------------------------------
// (the document of span s is span_doc_of over span_off: span_off[0] <= s < span_off[n_docs])

// span (start, len) of the document [a, b) of the text: 1 when the document is one (offsets ascend) and the span lies inside it
GFT_HD inline uint32_t redact_span_ok(uint64_t a, uint64_t b, uint32_t start, uint32_t len) {
    return (b >= a && (uint64_t)start + (uint64_t)len <= b - a) ? 1u : 0u;
}

// tiles of the fill pass over n spans
GFT_HD inline uint64_t redact_tiles(uint64_t n_spans) { return (n_spans + kSpanTile - 1) / kSpanTile; }

// the lane whose span holds virtual byte v of a tile: the last lane j with excl(j) <= v, where excl(j) = the summed lengths of
// the lanes in front of j (ascending, excl(0) = 0).  For v below the tile's sum that lane's span is not empty.  Every lane of a
// wave calls this together: excl(j) is a read of lane j's value.
template <class Excl>
GFT_HD inline uint32_t span_fill_lane(const Excl& excl, uint64_t v) {
    uint32_t lo = 0;
#pragma unroll
    for (uint32_t step = kSpanTile / 2; step; step >>= 1) {
        const uint64_t x = excl(lo + step);
        if (x <= v) lo += step;
    }
    return lo;
}

}  // namespace gft
