// gft_replace_piece.hpp -- replace: every hit run rewritten by its replacement (gft_replace_spans_device): what a plan entry, a
// window and a 16-byte chunk of the output decide, shared by the kernels (gft_replace.hip) and the host walk (replace_host.cpp).
//
// Runs.  The runs are the highlight's (gft_mark_piece.hpp): the excerpts of gft_excerpt_piece.hpp with before = after = 0 and no
// snap; the rank of a head over the whole batch is the number of its run.  A run's replacement is the smallest id its spans ask
// for (rep_span_id), whatever the order of the spans in the list.
//
// The plan.  Run j of the batch, [q0, q1) of the blob with a replacement of len bytes, has the entry
//     at(j)    = q0 - base + (replacement bytes of the runs in front) - (run bytes of the runs in front),   base = doc_off[0]
//     delta(j) = q1 - (at(j) + len): behind the replacement, up to the next entry, output position p is text[delta(j) + p]
//     len(j), roff(j): the replacement is tab[roff, roff + len)
// at ascends, but not strictly: at(j + 1) = at(j) + len(j) + (the text between the two runs), and deleted runs with no text
// between them -- on both sides of a document border -- give equal entries.  With n = the entries at or in front of output
// position p, entry n - 1 -- the LAST of its equals -- decides p: byte p - at of its replacement while that is below len, and
// text[delta + p] otherwise; with n == 0 the entry in front of the list decides, {at 0, len 0, delta base}.
//
// The copy is built from the OUTPUT side with the geometry of gft_select_piece.hpp: chunks of 16 bytes aligned to the output
// address, a lane a chunk, a wave a tile of kSelTrips trips.  One uniform search per tile finds n for the tile's first byte; the
// kRepWindow entries behind it lie across the lanes (where each begins, relative to the tile: mark_lift counts those at or in
// front of a chunk), and the entries that begin inside the tile lie in memory (LDS on the device) with all their fields, so that a
// chunk reads nothing of the plan from global memory.  A chunk that the entry in front of it has left and that ends at or in front
// of the next entry is PLAIN: one load at delta + lo.  Any other chunk is assembled segment by segment (rep_segment), a text
// segment or a replacement segment each with a load of its own: with deleted runs the text bytes of a chunk are NOT consecutive
// in the blob, sixteen one-byte pieces at worst.
#pragma once
#include <stdint.h>

#include "../../include/gft.h"
#include "gft_mark_piece.hpp"
#include "gft_select_piece.hpp"

namespace gft {

constexpr uint32_t kRepWindow = kMarkWindow;       // plan entries a wave holds across its lanes (mark_lift's width)
constexpr uint32_t kRepCtlGrow = 5;                // control word (behind the excerpt's): a document reaches 4 GiB once replaced
constexpr uint32_t kRepCtlKey = 6;                 // ... a key at or past n_keys, or an id at or past n_reps
constexpr uint32_t kRepMaxReps = 65536;            // entries of the table
constexpr uint32_t kRepNoId = 0xFFFFFFFFu;         // the minimum of no id
constexpr uint32_t kRepLdsTable = 4096;            // a table of this many bytes or fewer is staged in LDS by every workgroup
constexpr uint32_t kRepTableSlack = 32;            // zero bytes behind the table: sixteen bytes from any of its bytes are there

struct RepPlan {
    const uint64_t* at;            // [nr] where the run's replacement begins in the output
    const uint64_t* delta;         // [nr] text position minus output position behind the replacement (modulo 2^64)
    const uint32_t* len;           // [nr] bytes of the replacement
    const uint32_t* roff;          // [nr] where it begins in the table
    uint64_t nr;                   // runs
    uint64_t base;                 // doc_off[0]
};

struct RepEntry {
    uint64_t at, delta;
    uint32_t len, roff;
};

// the id span s asks for: kRepNoId when the key or the id is out of range
GFT_HD inline uint32_t rep_span_id(const uint32_t* span_key, const uint32_t* key_rep, uint32_t n_keys, uint32_t n_reps, uint64_t s) {
    uint32_t id = 0;
    if (span_key) {
        id = span_key[s];
        if (key_rep) {
            if (id >= n_keys) return kRepNoId;
            id = key_rep[id];
        }
    }
    return id < n_reps ? id : kRepNoId;
}
// a document of L bytes, `cut` of them in runs, with `put` bytes of replacements stays below 4 GiB
GFT_HD inline uint32_t rep_grow_ok(uint64_t L, uint64_t cut, uint64_t put) { return (L - cut + put < (1ull << 32)) ? 1u : 0u; }

GFT_HD inline RepEntry rep_entry(const RepPlan& R, uint64_t j) { return RepEntry{R.at[j], R.delta[j], R.len[j], R.roff[j]}; }
GFT_HD inline RepEntry rep_entry_none(const RepPlan& R) { return RepEntry{0, R.base, 0, 0}; }
// the entries that begin at or in front of output position p
GFT_HD inline uint64_t rep_count(const RepPlan& R, uint64_t p) {
    uint64_t a = 0, b = R.nr;                                       // at[j] <= p for j < a, at[j] > p for j >= b
    while (a < b) {
        const uint64_t mid = a + (b - a) / 2;
        if (R.at[mid] <= p) a = mid + 1; else b = mid;
    }
    return a;
}

// The window: entry w says where plan entry nb + w begins, relative to the tile's first position and cut to 32 bits, nb = the
// entries at or in front of that position -- so every entry is above 0 --; past the list: never reached (mark_window_rel's rule).
GFT_HD inline uint32_t rep_window_rel(const RepPlan& R, uint64_t nb, uint32_t w, uint64_t tile_lo) {
    if (nb + w >= R.nr) return 0xFFFFFFFFu;
    const uint64_t v = R.at[nb + w];
    return v <= tile_lo ? 0u : (v - tile_lo > 0xFFFFFFFEull ? 0xFFFFFFFEu : (uint32_t)(v - tile_lo));
}
// The window in memory, as a chunk reads it: rel as above; delta, len and roff of the entries that begin inside the tile (rel below
// `span`, the tile's bytes) -- the others are not stored and not read from here; front: entry nb - 1, or the entry in front of
// the list.
struct RepWin {
    const uint32_t* rel;           // [kRepWindow]
    const uint64_t* delta;         // [kRepWindow]
    const uint32_t* len;           // [kRepWindow]
    const uint32_t* roff;          // [kRepWindow]
    uint64_t nb, tile_lo;
    uint32_t span;
    RepEntry front;
};
GFT_HD inline RepEntry rep_entry_near(const RepPlan& R, const RepWin& W, uint64_t j) {
    if (j + 1 == W.nb) return W.front;
    if (j >= W.nb && j - W.nb < kRepWindow) {
        const uint64_t w = j - W.nb;
        const uint32_t r = W.rel[w];
        if (r != 0u && r < W.span) return RepEntry{W.tile_lo + r, W.delta[w], W.len[w], W.roff[w]};
    }
    return rep_entry(R, j);
}
GFT_HD inline uint64_t rep_at_near(const RepPlan& R, const RepWin& W, uint64_t j) {
    if (j >= W.nb && j - W.nb < kRepWindow) {
        const uint32_t r = W.rel[j - W.nb];
        if (r != 0u && r < 0xFFFFFFFEu) return W.tile_lo + r;
    }
    return R.at[j];
}

// The chunk [lo, hi) is plain: entry E decides lo (E = entry n - 1 of the n at or in front of lo), its replacement has ended
// at or in front of lo, and the next entry (next_rel, relative to the tile as hi_rel is) begins at or behind hi.  Its sixteen
// bytes are text[E.delta + lo ..] as they are.
GFT_HD inline bool rep_chunk_plain(const RepEntry& E, uint64_t lo, uint32_t next_rel, uint32_t hi_rel) {
    return E.at + E.len <= lo && next_rel >= hi_rel;
}

// where a chunk stands while it is assembled: the next position, the entries at or in front of it, its byte in the chunk
struct RepCursor {
    uint64_t p, n;
    uint32_t j;
};
// One segment at the cursor (c.p < hi): the rest of the replacement that c.p lies in, or the text up to the next entry, cut at
// hi; tab: the table (rep_off of the call laid end to end, kRepTableSlack bytes behind it).  A segment has a byte at least: c.p
// is below the replacement's end in the one case and below the next entry in the other.
GFT_HD inline void rep_segment(const RepPlan& R, const RepWin& W, const uint8_t* text, const uint8_t* tab, uint64_t hi, RepCursor& c, SelV& acc) {
    const RepEntry E = c.n ? rep_entry_near(R, W, c.n - 1) : rep_entry_none(R);
    const uint64_t off = c.p - E.at;
    uint64_t seg_end;
    SelV v;
    if (off < E.len) {
        seg_end = E.at + E.len < hi ? E.at + E.len : hi;
        v = sel_load(tab + (E.roff + off), (uint32_t)(seg_end - c.p));
    } else {
        const uint64_t next = c.n < R.nr ? rep_at_near(R, W, c.n) : ~0ull;
        seg_end = next < hi ? next : hi;
        v = sel_load(text + (E.delta + c.p), (uint32_t)(seg_end - c.p));
    }
    mark_or(acc, sel_shift(v, c.j));
    c.j += (uint32_t)(seg_end - c.p);
    c.p = seg_end;
    // the entries at or in front of the new position: a few steps as a rule; a long row of equal entries is searched
    for (uint32_t s = 0; c.n < R.nr && rep_at_near(R, W, c.n) <= c.p; s++) {
        if (s == 4) { c.n = rep_count(R, c.p); break; }
        c.n++;
    }
}

}  // namespace gft
