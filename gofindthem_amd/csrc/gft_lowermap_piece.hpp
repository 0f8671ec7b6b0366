// gft_lowermap_piece.hpp -- spans of a lowered batch mapped back to the source text (gft_map_spans_to_source_device): where a
// piece's table entry lies and what one span decides, shared by the kernels (gft_tolower.hip's table pass, gft_lowermap.hip) and
// the host walk (lowermap_host.cpp).
//
// The table.  The lower kernels walk a document in work units {doc, lo, hi} and a unit in 16-byte pieces from lo on; the table
// holds, for every piece, where its output begins in ITS DOCUMENT's lower-case form (uint32: such a form has less than 4 GiB).
// The piece j of unit u has the slot
//
//     ((doc_abs - doc_off[0] + lo) >> 4) + u + j          (lowermap_slot: u counts the batch's units)
//
// which needs no prefix sum over the pieces: a unit of n bytes that begins at text byte A fills slots up to
// (A >> 4) + ceil(n / 16) - 1 + u <= ((A + n) >> 4) + u, and unit u + 1 begins at or behind A + n with one more in u -- the runs
// never meet.  (Units of a long document are ceil(len / k) bytes, no multiple of 16, so a slot that counted documents instead of
// units would not do.)  The slots between two runs are never written and never read.  (text bytes >> 4) + units + 1 slots in all.
//
// The search.  A lowered byte x < B of document d: the last unit of d whose output begins at or before x (unit_out, the count
// pass's prefix sums: an empty unit shares its start with its successor and is never the answer), the last piece of that unit
// whose entry is <= x (the same holds for a piece without output: continuation bytes of a rune led from the piece in front), and
// the rune inside the piece by tolower_piece_rune_at.  B = unit_out[first unit of d + 1] - unit_out[first unit of d]: no sentinel
// entries are needed.
// Needs GFT_HD, Unit (gft_kernels.hpp).
#pragma once
#include <stdint.h>

#include "gft_kernels.hpp"
#include "gft_tolower_piece.hpp"

namespace gft {

constexpr uint32_t kMapTile = 64;          // spans a wave of the map passes takes per step: one per lane

GFT_HD inline uint64_t lowermap_slot(uint64_t unit_text_off, uint64_t u) { return (unit_text_off >> 4) + u; }
GFT_HD inline uint64_t lowermap_slots(uint64_t text_bytes, uint64_t n_units) { return (text_bytes >> 4) + n_units + 1; }

// what the search reads: the source batch, the unit table with the count pass's prefix sums, the pieces' table
struct LowerMapView {
    const uint8_t* text;
    const uint64_t* doc_off;       // [n_docs + 1]
    uint64_t n_docs;
    const uint64_t* unit_base;     // [n_docs + 1]   the first unit of every document
    const Unit* units;
    const uint64_t* unit_out;      // [n_units + 1]  where a unit's output begins in the lowered batch
    const uint32_t* tab;           // [lowermap_slots]
    LowerTable T;
};

// the lowered length of document d
GFT_HD inline uint64_t lowermap_doc_len(const LowerMapView& V, uint64_t d) { return V.unit_out[V.unit_base[d + 1]] - V.unit_out[V.unit_base[d]]; }

// the rune whose lower-case form holds byte x of document d's lowered form, x < lowermap_doc_len: a = its first source byte,
// relative to the document, sl = its source bytes
GFT_HD inline void lowermap_find(const LowerMapView& V, uint64_t d, uint32_t x, uint32_t& a, uint32_t& sl) {
    const uint64_t ub = V.unit_base[d], out0 = V.unit_out[ub];
    uint64_t lo = ub, hi = V.unit_base[d + 1] - 1;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (V.unit_out[mid] - out0 <= x) lo = mid;
        else hi = mid - 1;
    }
    const Unit un = V.units[lo];
    a = un.lo; sl = 0;
    if (un.hi <= un.lo) return;                                     // (not with x below the document's lowered length)
    const uint64_t doc_abs = V.doc_off[d], doc_len = V.doc_off[d + 1] - doc_abs;
    const uint32_t* tab = V.tab + lowermap_slot(doc_abs - V.doc_off[0] + un.lo, lo);
    uint32_t pl = 0, ph = (un.hi - un.lo + kLowerPiece - 1) / kLowerPiece - 1;
    while (pl < ph) {
        const uint32_t mid = pl + (ph - pl + 1) / 2;
        if (tab[mid] <= x) pl = mid;
        else ph = mid - 1;
    }
    const uint64_t o = (uint64_t)un.lo + (uint64_t)pl * kLowerPiece;
    LowerWin w;
    tolower_load_piece(V.text + doc_abs + o, o < 3 ? (uint32_t)o : 3u, doc_len - o, w);
    const uint32_t n = un.hi - o < kLowerPiece ? (uint32_t)(un.hi - o) : kLowerPiece;
    a = (uint32_t)o + tolower_piece_rune_at(V.T, w, n, x - tab[pl], sl);
}

// The lowered span (start, len) of document d as a span of the source: from the first byte of the rune that holds lowered byte
// `start` to the last byte of the rune that holds lowered byte start + len - 1.  len == 0: (that rune's first byte, 0); at the
// lowered end: (the document's length, 0).  Returns 0, and decides nothing, for a span that reaches past the lowered end.
GFT_HD inline uint32_t lowermap_span(const LowerMapView& V, uint64_t d, uint32_t start, uint32_t len, uint32_t& s_start, uint32_t& s_len) {
    const uint64_t B = lowermap_doc_len(V, d);
    if ((uint64_t)start + (uint64_t)len > B) return 0u;
    s_len = 0;
    if (start == B) { s_start = (uint32_t)(V.doc_off[d + 1] - V.doc_off[d]); return 1u; }
    uint32_t a, sl;
    lowermap_find(V, d, start, a, sl);
    s_start = a;
    if (!len) return 1u;
    uint32_t a2 = a, sl2 = sl;
    if (len > 1) lowermap_find(V, d, start + (len - 1), a2, sl2);
    s_len = a2 + sl2 - a;
    return 1u;
}

}  // namespace gft
