// gft_mark_piece.hpp -- highlight: markers written round the hit spans (gft_mark_spans_device): what the insertion list says, and
// what a tile, a window and a 16-byte chunk of the output decide, shared by the kernels (gft_mark.hip) and the host walk
// (mark_host.cpp).
//
// Runs.  The runs of a document are the connected components of the union of its spans, touching spans joined: the excerpts of
// gft_excerpt_piece.hpp with before = after = 0 and no snap.  Its window pass, suffix minimum and head rule are used as they are;
// the rank of a head over the whole batch is the number of its run.
//
// The insertion list.  With R runs in the batch, insertion j (0 <= j < 2R) is `open` for even j and `close` for odd j, and sits
// at blob position q[j]: the start of run j >> 1 for even j, its end for odd j.  q ascends (runs are apart inside a document, and
// a later document's runs lie at or behind this document's end).  ins(n) = bytes that the first n insertions add; insertion j
// begins in the output at
//     at(j) = q[j] - base + ins(j),          base = doc_off[0]
// which ascends too, strictly wherever the marker in front has a byte.  Output position p, with n = the insertions that begin at
// or in front of p, is byte p - at(n - 1) of marker n - 1 when that is below its length, and text[base + p - ins(n)] otherwise:
// between two insertions the text is a straight copy at a known shift.
//
// The copy is built from the OUTPUT side with the geometry of gft_select_piece.hpp: chunks of 16 bytes aligned to the output
// address, a lane a chunk, a wave a tile of kSelTrips trips.  One uniform search per tile finds n for the tile's first byte; the
// kMarkWindow insertions behind it lie across the lanes (where each begins, relative to the tile), and a lane counts those at or
// in front of its chunk with shuffles; the two entries round that count say whether the chunk holds an insertion at all.  Every
// chunk loads its text once, at most sixteen consecutive bytes of the blob (mark_chunk_src); one without an insertion stores them
// as they are, one with insertions spreads them round the marker bytes in registers, with the positions from the window's copy in
// memory and nothing more from global memory.  A chunk that the window cannot place (more than kMarkWindow - 2 insertions between the tile's first byte and the chunk) searches the list itself.
#pragma once
#include <stdint.h>

#include "../../include/gft.h"
#include "gft_select_piece.hpp"

namespace gft {

constexpr uint32_t kMarkWindow = 64;               // insertions a wave holds across its lanes
constexpr uint32_t kMarkSlot = 256;                // bytes of a marker's slot in the marker block: open at 0, close at kMarkSlot
constexpr uint32_t kMarkWords = 2 * kMarkSlot / 8 + 2;  // the block as 64-bit words, two more so that 16 bytes from any marker byte are there
constexpr uint32_t kMarkCtlGrow = 5;               // control word (behind the excerpt's): a document reaches 4 GiB once marked

struct MarkPlan {
    const uint64_t* q;             // [nq] the insertion list, blob positions
    uint64_t nq;                   // 2 * runs
    uint64_t base;                 // doc_off[0]
    uint64_t text_len;             // doc_off[n_docs] - doc_off[0]
    uint32_t ol, cl;               // bytes of open and of close
};

// the bytes that the first n insertions add
GFT_HD inline uint64_t mark_ins(const MarkPlan& M, uint64_t n) { return ((n + 1) >> 1) * M.ol + (n >> 1) * M.cl; }
GFT_HD inline uint32_t mark_len(const MarkPlan& M, uint64_t j) { return (j & 1) ? M.cl : M.ol; }
// where insertion j begins in the output
GFT_HD inline uint64_t mark_at(const MarkPlan& M, uint64_t j) { return M.q[j] - M.base + mark_ins(M, j); }
// the insertions that begin at or in front of output position p
GFT_HD inline uint64_t mark_count(const MarkPlan& M, uint64_t p) {
    uint64_t a = 0, b = M.nq;                                       // at(j) <= p for j < a, at(j) > p for j >= b
    while (a < b) {
        const uint64_t mid = a + (b - a) / 2;
        if (mark_at(M, mid) <= p) a = mid + 1; else b = mid;
    }
    return a;
}
// a span's start in its marked document: r is the index of its run within the document
GFT_HD inline uint32_t mark_span_new(uint32_t start, uint64_t r, uint32_t ol, uint32_t cl) {
    return (uint32_t)(start + (r + 1) * ol + r * cl);
}
// a document of L bytes with r runs stays below 4 GiB once marked
GFT_HD inline uint32_t mark_grow_ok(uint64_t L, uint64_t r, uint32_t ol, uint32_t cl) {
    return (r <= (1ull << 32) && L + r * ((uint64_t)ol + cl) < (1ull << 32)) ? 1u : 0u;
}

// The window: entry w says where insertion nb + w begins, relative to the tile's first position and cut to 32 bits, nb = the
// insertions at or in front of that position -- so every entry is above 0 --; past the list: never reached.
GFT_HD inline uint32_t mark_window_rel(const MarkPlan& M, uint64_t nb, uint32_t w, uint64_t tile_lo) {
    if (nb + w >= M.nq) return 0xFFFFFFFFu;
    const uint64_t v = mark_at(M, nb + w);
    return v <= tile_lo ? 0u : (v - tile_lo > 0xFFFFFFFEull ? 0xFFFFFFFEu : (uint32_t)(v - tile_lo));
}
// The entries at or below p_rel, for ascending entries: 0 .. kMarkWindow - 2 is the count itself; kMarkWindow - 1: that many or
// more, the window does not say.  rel(w): entry w -- a shuffle across the lanes on the device (every lane of the wave makes every
// call), an array on the host.
template <class At>
GFT_HD inline uint32_t mark_lift(const At& rel, uint32_t p_rel) {
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t s = kMarkWindow / 2; s; s >>= 1) {
        const uint32_t v = rel(cnt + s - 1);
        if (v <= p_rel) cnt += s;
    }
    return cnt;
}

// where the insertion in front of the window begins in the output (0: none)
GFT_HD inline uint64_t mark_window_front(const MarkPlan& M, uint64_t nb) { return nb ? mark_at(M, nb - 1) : 0; }
// The text of a chunk.  The output is the batch's text in order with the markers in between, so the text bytes of a chunk
// [lo, hi) are ONE run of at most hi - lo consecutive bytes of the blob, whatever lies between them in the output: from
// blob position base + src, src = the text bytes of the output in front of lo.  n insertions begin at or in front of lo, the last
// of them at prev_at: lo lies inside that marker, or behind it.
GFT_HD inline uint64_t mark_chunk_src(const MarkPlan& M, uint64_t n, uint64_t prev_at, uint64_t lo) {
    return (n && lo < prev_at + mark_len(M, n - 1)) ? prev_at - mark_ins(M, n - 1) : lo - mark_ins(M, n);
}
// ... loaded once, for every chunk alike: aligned 16-byte loads and the byte-align funnel (sel_load); never past the text's end
GFT_HD inline SelV mark_chunk_text(const MarkPlan& M, const uint8_t* text, uint64_t src, uint64_t lo, uint64_t hi) {
    const uint64_t left = M.text_len - src, n = left < hi - lo ? left : hi - lo;
    return n ? sel_load(text + (M.base + src), (uint32_t)n) : SelV{0, 0};
}
// The chunk holds no insertion -- the common case, decided from the window alone: the insertion in front of it has ended and the
// next one (next_rel, relative to the tile as hi_rel is) begins at or behind its end.  Its text goes to byte j as it is.
GFT_HD inline bool mark_chunk_plain(const MarkPlan& M, uint64_t n, uint64_t prev_at, uint64_t lo, uint32_t next_rel, uint32_t hi_rel) {
    return (n == 0 || prev_at + mark_len(M, n - 1) <= lo) && next_rel >= hi_rel;
}
// v moved k bytes towards the start of the chunk (0 <= k <= 15)
GFT_HD inline SelV mark_drop(SelV v, uint32_t k) {
    if (k == 0) return v;
    if (k >= 8) return SelV{v.hi >> (8 * (k - 8)), 0};
    return SelV{(v.lo >> (8 * k)) | (v.hi << (64 - 8 * k)), v.hi >> (8 * k)};
}

// The window as a chunk that meets insertions reads it: the entries in memory (LDS on the device), so that where an insertion of
// the tile begins costs no load from the list; an insertion outside the window, or one the 32-bit cut hides, is read from the list.
struct MarkWin {
    const uint32_t* rel;           // [kMarkWindow] mark_window_rel of nb, nb + 1, ...
    uint64_t nb, tile_lo;
};
GFT_HD inline uint64_t mark_at_near(const MarkPlan& M, const MarkWin& W, uint64_t j) {
    if (j >= W.nb && j - W.nb < kMarkWindow) {
        const uint32_t r = W.rel[j - W.nb];
        if (r != 0u && r < 0xFFFFFFFEu) return W.tile_lo + r;
    }
    return mark_at(M, j);
}

// where a chunk stands while it is assembled: the next position, the insertions at or in front of it, its byte in the chunk
struct MarkCursor {
    uint64_t p, n;
    uint32_t j;
};
GFT_HD inline void mark_or(SelV& acc, const SelV& v) { acc.lo |= v.lo; acc.hi |= v.hi; }
GFT_HD inline void mark_advance(const MarkPlan& M, const MarkWin& W, MarkCursor& c) {
    while (c.n < M.nq && mark_at_near(M, W, c.n) <= c.p) c.n++;
}
// position c.p lies in marker c.n - 1
GFT_HD inline bool mark_in_marker(const MarkPlan& M, const MarkWin& W, const MarkCursor& c) {
    return c.n > 0 && c.p < mark_at_near(M, W, c.n - 1) + mark_len(M, c.n - 1);
}
// The text segment at the cursor, up to the next insertion or hi: the next bytes of the chunk's text T, `used` of which are
// placed already.  Asks for a cursor that is not in a marker and c.p < hi.
GFT_HD inline void mark_text_segment(const MarkPlan& M, const MarkWin& W, const SelV& T, uint32_t& used, uint64_t hi, MarkCursor& c, SelV& acc) {
    const uint64_t next = c.n < M.nq ? mark_at_near(M, W, c.n) : ~0ull;
    const uint64_t seg_end = next < hi ? next : hi;
    const uint32_t len = (uint32_t)(seg_end - c.p);
    mark_or(acc, sel_shift(sel_keep(mark_drop(T, used), len), c.j));
    used += len;
    c.j += len;
    c.p = seg_end;
    mark_advance(M, W, c);
}
// The marker segment at the cursor, up to the marker's end or hi.  marks: the marker block as words, open at byte 0 and close at
// byte kMarkSlot: the sixteen bytes from the marker's next byte on are three words through the funnel.
GFT_HD inline void mark_marker_segment(const MarkPlan& M, const MarkWin& W, const uint64_t* marks, uint64_t hi, MarkCursor& c, SelV& acc) {
    const uint64_t j = c.n - 1, at = mark_at_near(M, W, j), end = at + mark_len(M, j);
    const uint64_t seg_end = end < hi ? end : hi;
    const uint32_t k = (uint32_t)(c.p - at), len = (uint32_t)(seg_end - c.p);
    const uint64_t* m = marks + ((j & 1) ? kMarkSlot / 8 : 0u) + (k >> 3);
    const uint64_t a = m[0], b = m[1], d = m[2];
    const SelV v{sel_funnel(a, b, k & 7u), sel_funnel(b, d, k & 7u)};
    mark_or(acc, sel_shift(sel_keep(v, len), c.j));
    c.j += len;
    c.p = seg_end;
    mark_advance(M, W, c);
}
// A chunk that meets insertions, from the cursor on: markers and text in turn
GFT_HD inline void mark_chunk_rest(const MarkPlan& M, const MarkWin& W, const SelV& T, const uint64_t* marks, uint64_t hi, MarkCursor c, SelV& acc) {
    uint32_t used = 0;
    while (c.p < hi) {
        if (mark_in_marker(M, W, c)) mark_marker_segment(M, W, marks, hi, c, acc);
        else mark_text_segment(M, W, T, used, hi, c, acc);
    }
}

}  // namespace gft
