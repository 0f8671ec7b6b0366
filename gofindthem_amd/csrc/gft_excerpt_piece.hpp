// gft_excerpt_piece.hpp -- excerpts: the text around the hit spans, cut and gathered (gft_excerpt_spans_device): what a window, the
// rune snap and a cut are, and what a tile, a carry trip and a lane decide, shared by the kernels (gft_excerpt.hip) and the host
// walk (excerpt_host.cpp).
//
// Windows.  Span (start, len) of document d = [a, b) of the text, L = b - a, has the window [max(0, start - before),
// min(L, start + len + after)) of the document, in 64 bits.  With GFT_EXCERPT_RUNES its start moves back while the byte AT the start
// is a UTF-8 continuation byte and its end forward while the byte AT the end is one, three steps each at most and never past the
// document's first byte or its end: only bytes of the document itself are read.  The kernels work in positions of the blob:
// ws = a + window start, we = a + window end.
//
// Snaps (gft_excerpt_spans_snap_device).  With GFT_EXCERPT_WORDS (which implies the rune snap: an edge inside a rune cuts no word
// while its neighbours do, and the rule would not be monotone) the start then steps back and the end forward, a rune a step,
// while the edge CUTS A WORD -- word(DecodeLastRune(D[:p])) and word(DecodeRune(D[p:])), the predicate and decoders of
// gft_words_piece.hpp --; with GFT_EXCERPT_LINES they step a byte at a time until they stand behind a '\n' / on one.  An edge
// that would move more than `reach` bytes stays where it began.  Both only grow a window, are monotone in the edge they start
// from and read single bytes of the document alone, so everything below holds for snapped windows as it stands.
//
// Cuts.  The spans' ends ascend inside a document, so do the windows' (clipping and the snap are monotone), and with them the
// excerpts -- the connected components of the union of a document's windows, touching windows joined -- are runs of consecutive
// spans.  With smin(k) = min of ws over the spans k, k + 1, ... of the whole batch (a later document's windows begin at or behind
// this document's end, so they never lower the minimum below a window of this one):
//     span k is the HEAD of an excerpt   iff  it is the first span of its document or we(k - 1) < smin(k)
//     the excerpt of head k begins at smin(k) and ends at we of the last span in front of the next head.
// Its length is spread over its spans -- we(k) - smin(k) at the head, we(k) - we(k - 1) behind it, each below 4 GiB -- so that one
// exclusive prefix sum gives every head its excerpt's offset in the output, and one over the head flags its rank.
//
// Suffix minimum.  A tile is kExcTile consecutive spans, a lane each; a carry trip kExcCarryTiles consecutive tiles, a lane each.
// The window pass leaves every tile's minimum; one workgroup walks the trips from the last to the first and leaves in front of
// every tile the minimum of all tiles behind it (the carry); the mark pass scans its tile from that carry.  Inside a wave the scan
// is exc_scan_step over the distances 1, 2, .. 32; the waves of a workgroup meet in exc_later.
#pragma once
#include <stdint.h>

#include "../../include/gft.h"
#include "gft_select_piece.hpp"
#include "gft_spans_piece.hpp"
#include "gft_words_piece.hpp"

namespace gft {

constexpr uint32_t kExcTile = 256;                 // spans of a tile: a workgroup of the window and the mark pass, a lane a span
constexpr uint32_t kExcCarryTiles = 1024;          // tiles of a carry trip: the one workgroup of the carry pass, a lane a tile
constexpr uint64_t kExcNone = ~0ull;               // the minimum of no window
// what a lane of the window pass finds wrong (exc_lane_window)
constexpr uint64_t kExcBadSpan = 1;                // a span past its document's end, or ends that descend inside a document
constexpr uint64_t kExcBadDoc = 2;                 // document offsets descend, or a document of 4 GiB or more
// the control block's words.  A refusal is one word a condition, and every lane that meets the condition stores the same 1
constexpr uint32_t kExcCtlExc = 0, kExcCtlTotal = 1;   // the excerpts and their bytes
constexpr uint32_t kExcCtlDocs = 2;                // the document pass refuses: the passes behind it store nothing
constexpr uint32_t kExcCtlSpans = 3;               // the window pass refuses: a span past its document's end, or ends that descend
constexpr uint32_t kExcCtlOffs = 4;                // ... and what the document pass met was span offsets that descend
constexpr uint32_t kExcCtlEnds = 8;                // span_off[0], span_off[n_docs], doc_off[0], doc_off[n_docs]
constexpr uint32_t kExcCtlWords = 12;

GFT_HD inline uint64_t exc_tiles(uint64_t n_spans) { return (n_spans + kExcTile - 1) / kExcTile; }
GFT_HD inline uint64_t exc_trips(uint64_t n_tiles) { return (n_tiles + kExcCarryTiles - 1) / kExcCarryTiles; }

// ---- what a window is -------------------------------------------------------------------------------------------------------
GFT_HD inline bool exc_is_cont(uint8_t b) { return (b & 0xC0u) == 0x80u; }

// the window [lo, hi) of span (start, len) in a document of L bytes, before the snap.  0 <= lo <= hi <= L whatever the span says.
GFT_HD inline void exc_window(uint64_t L, uint32_t start, uint32_t len, uint32_t before, uint32_t after, uint64_t& lo, uint64_t& hi) {
    lo = start > before ? (uint64_t)start - before : 0;
    hi = (uint64_t)start + len + after;
    if (lo > L) lo = L;
    if (hi > L) hi = L;
}
// the snap: doc[0, L) is the document; nothing outside it is read
GFT_HD inline uint64_t exc_snap_start(const uint8_t* doc, uint64_t L, uint64_t lo) {
    for (uint32_t s = 0; s < 3 && lo > 0 && lo < L && exc_is_cont(doc[lo]); s++) lo--;
    return lo;
}
GFT_HD inline uint64_t exc_snap_end(const uint8_t* doc, uint64_t L, uint64_t hi) {
    for (uint32_t s = 0; s < 3 && hi < L && exc_is_cont(doc[hi]); s++) hi++;
    return hi;
}
// the word snap.  The rune stepped over was decoded as the far side of the cut before: every rune of the walk is decoded once.
GFT_HD inline uint64_t exc_word_start(const WordTable& T, const uint8_t* doc, uint64_t L, uint64_t lo, uint32_t reach) {
    if (lo == 0 || lo >= L || !words_first_is_word(T, doc + lo, L - lo)) return lo;
    uint64_t p = lo;
    while (p > 0) {                                                 // (a word rune begins at p)
        const uint32_t r = words_last_word_size(T, doc, p);
        if (!r) break;
        if (lo - (p - r) > reach) return lo;                        // the word is longer than the reach: given up
        p -= r;
    }
    return p;
}
GFT_HD inline uint64_t exc_word_end(const WordTable& T, const uint8_t* doc, uint64_t L, uint64_t hi, uint32_t reach) {
    if (hi == 0 || hi >= L || !words_last_is_word(T, doc, hi)) return hi;
    uint64_t p = hi;
    while (p < L) {                                                 // (a word rune ends at p)
        const uint32_t r = words_first_word_size(T, doc + p, L - p);
        if (!r) break;
        if ((p + r) - hi > reach) return hi;
        p += r;
    }
    return p;
}
// the line snap: the start behind a newline or at 0, the end on a newline or at L
GFT_HD inline uint64_t exc_line_start(const uint8_t* doc, uint64_t L, uint64_t lo, uint32_t reach) {
    (void)L;
    uint64_t p = lo;
    while (p > 0 && doc[p - 1] != '\n') {
        if (lo - (p - 1) > reach) return lo;
        p--;
    }
    return p;
}
GFT_HD inline uint64_t exc_line_end(const uint8_t* doc, uint64_t L, uint64_t hi, uint32_t reach) {
    uint64_t p = hi;
    while (p < L && doc[p] != '\n') {
        if ((p + 1) - hi > reach) return hi;
        p++;
    }
    return p;
}
// the flags and the reach of a snapped call are ones the call takes
GFT_HD inline bool exc_snap_args_ok(uint32_t flags, uint32_t reach) {
    if (flags & ~(uint32_t)(GFT_EXCERPT_RUNES | GFT_EXCERPT_WORDS | GFT_EXCERPT_LINES)) return false;
    if ((flags & GFT_EXCERPT_WORDS) && (flags & GFT_EXCERPT_LINES)) return false;
    return reach <= GFT_EXCERPT_REACH_MAX;
}
// the snaps of a clipped window [lo, hi) of doc[0, L), in the contract's order.  kSnap false: the rune snap alone
template <bool kSnap>
GFT_HD inline void exc_snap_window(const WordTable& T, const uint8_t* doc, uint64_t L, uint32_t flags, uint32_t reach, uint64_t& lo, uint64_t& hi) {
    if (flags & (GFT_EXCERPT_RUNES | (kSnap ? GFT_EXCERPT_WORDS : 0u))) {
        lo = exc_snap_start(doc, L, lo);
        hi = exc_snap_end(doc, L, hi);
    }
    if (!kSnap) return;
    if (flags & GFT_EXCERPT_WORDS) {
        lo = exc_word_start(T, doc, L, lo, reach);
        hi = exc_word_end(T, doc, L, hi, reach);
    } else if (flags & GFT_EXCERPT_LINES) {
        lo = exc_line_start(doc, L, lo, reach);
        hi = exc_line_end(doc, L, hi, reach);
    }
}
// span (start, len) lies inside a document of L bytes
GFT_HD inline uint32_t exc_span_ok(uint64_t L, uint32_t start, uint32_t len) { return ((uint64_t)start + len <= L) ? 1u : 0u; }
// the end of a span is not in front of the end of the span before it (same document)
GFT_HD inline uint32_t exc_order_ok(uint32_t prev_start, uint32_t prev_len, uint32_t start, uint32_t len) {
    return ((uint64_t)prev_start + prev_len <= (uint64_t)start + len) ? 1u : 0u;
}

struct ExcView {
    const uint8_t* text;
    const uint64_t* doc_off;       // [n_docs + 1]
    uint64_t n_docs;
    const uint64_t* span_off;      // [n_docs + 1]
    const uint32_t* span_start;
    const uint32_t* span_len;
    uint32_t before, after, flags;
    uint32_t reach;                // the snapped call's; 0 and an empty table: the plain call
    WordTable words;               // GFT_EXCERPT_WORDS: the class table (the device copy in the kernels)
};

// the window pass's lane: span s (span_off[0] <= s < span_off[n_docs]) -> its document, its snapped window in blob positions, and
// the flag bits it raises.  A refused span still gets a window inside its document, so that nothing behind it reads astray.
// kSnap: the word or line snap of V.flags behind the rune snap; false: the plain call's lane, which knows neither.
template <bool kSnap>
GFT_HD inline uint64_t exc_lane_window_t(const ExcView& V, uint64_t s, uint64_t& d, uint64_t& ws, uint64_t& we) {
    d = span_doc_of(V.span_off, V.n_docs, s);
    const uint64_t a = V.doc_off[d], b = V.doc_off[d + 1];
    if (!sel_doc_ok(a, b)) { ws = we = a; return kExcBadDoc; }
    const uint64_t L = b - a;
    const uint32_t start = V.span_start[s], len = V.span_len[s];
    uint64_t bad = exc_span_ok(L, start, len) ? 0 : kExcBadSpan;
    if (s > V.span_off[d] && !exc_order_ok(V.span_start[s - 1], V.span_len[s - 1], start, len)) bad |= kExcBadSpan;
    uint64_t lo, hi;
    exc_window(L, start, len, V.before, V.after, lo, hi);
    exc_snap_window<kSnap>(V.words, V.text + a, L, V.flags, V.reach, lo, hi);
    ws = a + lo;
    we = a + hi;
    return bad;
}
GFT_HD inline uint64_t exc_lane_window(const ExcView& V, uint64_t s, uint64_t& d, uint64_t& ws, uint64_t& we) {
    return exc_lane_window_t<false>(V, s, d, ws, we);
}

// ---- the suffix minimum -------------------------------------------------------------------------------------------------------
GFT_HD inline uint64_t exc_min(uint64_t a, uint64_t b) { return a < b ? a : b; }
// one step of a wave's inclusive suffix-minimum scan: `other` is the value of lane + step (any value where that is no lane)
GFT_HD inline uint64_t exc_scan_step(uint64_t self, uint64_t other, uint32_t lane, uint32_t step) {
    return lane + step < 64 ? exc_min(self, other) : self;
}
// what lies behind wave w of a workgroup of n_waves: the minima of the waves behind it (tot[w'] = what lane 0 of wave w' holds
// after the scan) and the carry in front of the workgroup.  w = -1: behind nothing, the minimum of it all -- the next carry.
GFT_HD inline uint64_t exc_later(const uint64_t* tot, uint32_t n_waves, int w, uint64_t carry) {
    uint64_t m = carry;
    for (uint32_t j = (uint32_t)(w + 1); j < n_waves; j++) m = exc_min(m, tot[j]);
    return m;
}
// a lane's exclusive suffix minimum from the wave's scan: `next` is lane + 1's inclusive value, `later` exc_later of its wave
GFT_HD inline uint64_t exc_exclusive(uint64_t next, uint64_t later, uint32_t lane) { return lane < 63 ? exc_min(next, later) : later; }

// ---- what a lane of the mark pass decides ----------------------------------------------------------------------------------------
// span k (first: of its document, or of the batch) with window end we, the window end of the span before it and smin(k)
GFT_HD inline uint32_t exc_is_head(bool first, uint64_t prev_we, uint64_t smin) { return (first || prev_we < smin) ? 1u : 0u; }
// its share of its excerpt's length
GFT_HD inline uint32_t exc_share(uint32_t head, uint64_t we, uint64_t prev_we, uint64_t smin) { return (uint32_t)(we - (head ? smin : prev_we)); }

}  // namespace gft
