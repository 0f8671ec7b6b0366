// gft_select_piece.hpp -- the documents that matched, gathered into one blob (gft_select_docs_device): what a row, a 16-byte chunk of
// the output and a window of compact offsets say, shared by the kernels (gft_select.hip) and the host walk (select_host.cpp).
//
// The copy is built from the OUTPUT side.  The output range [0, end), end = min(total, cap_bytes), is cut into chunks of 16 bytes
// aligned to the output ADDRESS: with a = address of d_out & 15, chunk c holds the positions [16c - a, 16c + 16 - a) that lie in
// [0, end).  A lane takes a chunk, a wave's trip 64 chunks, a wave a tile of kSelTrips trips.  The selected documents are the
// compact arrays c_off [m + 1] (where each starts in the output, c_off[m] = total; never capped) and c_src [m] (where it starts
// in the text).  The document of a position p is the k with c_off[k] <= p < c_off[k + 1] -- unique, empty documents included,
// because the one that holds p is the last of its run of equal offsets.
//
// A chunk is assembled in a SelV (sixteen bytes, byte i at bits 8i) from the segments of the documents that meet it -- one in
// the common case -- and stored with one 16-byte store when all its sixteen positions are in range, byte by byte otherwise (the
// first and the last chunk of the range: nothing outside [d_out, d_out + end) is written).
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/gft.h"

#ifndef GFT_HD
#if defined(__HIPCC__)
#define GFT_HD __host__ __device__
#else
#define GFT_HD
#endif
#endif

namespace gft {

constexpr uint32_t kSelChunk = 16;                         // bytes per lane and trip: one 16-byte store
constexpr uint32_t kSelTrip = 64 * kSelChunk;              // bytes per wave and trip
constexpr uint32_t kSelTrips = 4;                          // trips per tile: their loads are issued before the first store
constexpr uint32_t kSelTile = kSelTrips * kSelTrip;        // a wave's run of the output: 4 KiB
constexpr uint32_t kSelWindow = 64;                        // compact offsets a wave holds across its lanes

// ---- the mark pass: one word of a row against the same word of `want` (already cut to n_cols) -----------------------------
struct SelRow {
    uint32_t any, all;     // some wanted bit is set; no wanted bit is missing
};
GFT_HD inline SelRow sel_row_word(uint32_t w, uint32_t want) { return SelRow{(w & want) ? 1u : 0u, ((w & want) == want) ? 1u : 0u}; }
GFT_HD inline SelRow sel_row_join(SelRow a, SelRow b) { return SelRow{a.any | b.any, a.all & b.all}; }
// (the row of no words: any = 0, all = 1 -- n_cols == 0 selects nothing under ANY and everything under ALL and NONE)
GFT_HD inline uint32_t sel_row_decide(SelRow r, uint32_t mode) {
    return mode == GFT_SELECT_ANY ? r.any : mode == GFT_SELECT_ALL ? r.all : 1u - r.any;
}
// the document [a, b) of the offsets: 0 when they descend or it has 4 GiB or more
GFT_HD inline uint32_t sel_doc_ok(uint64_t a, uint64_t b) { return (b >= a && b - a < (1ull << 32)) ? 1u : 0u; }

// ---- the control block the host reads back: the select's words, then the two the context call adds -------------------------
// (bytes, documents kept, doc_off[0], doc_off[n_docs]; flag: offsets descend, or a document of 4 GiB or more)
enum : uint32_t {
    kSelCtlTotal = 0, kSelCtlM = 1, kSelCtlLo = 2, kSelCtlHi = 3, kSelCtlFlag = 4, kSelCtlWords = 5,
    kCtxCtlHits = 5, kCtxCtlGroups = 6, kCtxCtlWords = 7
};

// ---- the place pass: P is a parameter block with doc_off, pos, rank, c_off, c_src, out_off, doc_idx, cap_docs ----------------
// what the host walks place through
struct SelPlace {
    const uint64_t *doc_off, *pos, *rank;
    uint64_t *c_off, *c_src, *out_off, *doc_idx;
    uint64_t cap_docs;
};
// document d, if it is kept: the compact arrays (complete), the caller's out_off / doc_idx (capped); r: its rank
template <class P>
GFT_HD inline bool sel_place_doc(const P& p, uint64_t d, uint64_t& r) {
    r = p.rank[d];
    if (p.rank[d + 1] == r) return false;
    const uint64_t at = p.pos[d];
    p.c_off[r] = at;
    p.c_src[r] = p.doc_off[d];
    if (p.out_off && r <= p.cap_docs) p.out_off[r] = at;
    if (r < p.cap_docs) p.doc_idx[r] = d;
    return true;
}
// the closing entries behind the m kept documents
template <class P>
GFT_HD inline void sel_place_close(const P& p, uint64_t m, uint64_t total) {
    p.c_off[m] = total;
    if (p.out_off && m <= p.cap_docs) p.out_off[m] = total;
}

// ---- the copy pass ---------------------------------------------------------------------------------------------------------
struct SelGeom {
    uint64_t end;          // bytes to write: min(total, cap_bytes)
    uint32_t a;            // the output address & 15
};
// the geometry of a call that has `total` bytes for an output of cap_bytes at `out`
inline SelGeom sel_geom(uint64_t total, uint64_t cap_bytes, const void* out) {
    return SelGeom{total < cap_bytes ? total : cap_bytes, (uint32_t)((uintptr_t)out & 15u)};
}
GFT_HD inline uint64_t sel_chunks(const SelGeom& G) { return G.end ? (G.end + G.a + kSelChunk - 1) / kSelChunk : 0; }
GFT_HD inline uint64_t sel_tiles(const SelGeom& G) { return (sel_chunks(G) + kSelTile / kSelChunk - 1) / (kSelTile / kSelChunk); }
// chunk c's positions [lo, hi); lo == hi: none (c is past the range)
GFT_HD inline void sel_chunk_range(const SelGeom& G, uint64_t c, uint64_t& lo, uint64_t& hi) {
    lo = c ? c * kSelChunk - G.a : 0;
    hi = (c + 1) * kSelChunk - G.a;
    if (hi > G.end) hi = G.end;
    if (lo > hi) lo = hi;
}
// the byte of chunk c that position p is
GFT_HD inline uint32_t sel_chunk_byte(const SelGeom& G, uint64_t c, uint64_t p) { return (uint32_t)(p + G.a - c * kSelChunk); }

struct SelV {
    uint64_t lo, hi;
};
// the first n bytes of v (1 <= n <= 16)
GFT_HD inline SelV sel_keep(SelV v, uint32_t n) {
    if (n >= 16) return v;
    if (n > 8) return SelV{v.lo, v.hi & (~0ull >> (128 - 8 * n))};
    return SelV{n == 8 ? v.lo : v.lo & (~0ull >> (64 - 8 * n)), 0};
}
// v moved j bytes towards the end of the chunk (0 <= j <= 15)
GFT_HD inline SelV sel_shift(SelV v, uint32_t j) {
    if (j == 0) return v;
    if (j >= 8) return SelV{0, v.lo << (8 * (j - 8))};
    return SelV{v.lo << (8 * j), (v.hi << (8 * j)) | (v.lo >> (64 - 8 * j))};
}
// x's bytes from byte s on, then y's (0 <= s <= 7): the byte-align funnel on 64-bit halves
GFT_HD inline uint64_t sel_funnel(uint64_t x, uint64_t y, uint32_t s) { return s ? (x >> (8 * s)) | (y << (64 - 8 * s)) : x; }
// n bytes at p (1 <= n <= 16), p unaligned.  The device assembles them from the aligned 16-byte granules round them: the one p
// lies in, and the next one when a byte of it is needed -- an aligned load never leaves the granule of a byte it needs, so a read
// in front of the blob stays in the blob's own granule and a read behind its end in the 64 bytes of slack.  The host reads its n
// bytes and nothing else.
GFT_HD inline SelV sel_load(const uint8_t* p, uint32_t n) {
    SelV v{0, 0};
#if defined(__HIP_DEVICE_COMPILE__)
    struct __attribute__((aligned(16))) U128a { uint64_t lo, hi; };
    const uint32_t r = (uint32_t)((uintptr_t)p & 15u);
    const U128a* g = reinterpret_cast<const U128a*>(p - r);
    const U128a a = g[0];
    U128a b{0, 0};
    if (r + n > 16) b = g[1];
    const uint32_t s = r & 7u;
    v.lo = r < 8 ? sel_funnel(a.lo, a.hi, s) : sel_funnel(a.hi, b.lo, s);
    v.hi = r < 8 ? sel_funnel(a.hi, b.lo, s) : sel_funnel(b.lo, b.hi, s);
#else
    uint8_t b[16] = {0};
    memcpy(b, p, n);
    for (uint32_t i = 0; i < 8; i++) { v.lo |= (uint64_t)b[i] << (8 * i); v.hi |= (uint64_t)b[8 + i] << (8 * i); }
#endif
    return sel_keep(v, n);
}

// the largest k with c_off[k] <= p; asks for c_off[0] <= p < c_off[m]
GFT_HD inline uint64_t sel_search(const uint64_t* c_off, uint64_t m, uint64_t p) {
    uint64_t a = 0, b = m;
    while (b - a > 1) {
        const uint64_t mid = a + (b - a) / 2;
        if (c_off[mid] <= p) a = mid; else b = mid;
    }
    return a;
}
// The window: kSelWindow consecutive compact documents from `base` on, a lane each.  Entry j says where document base + j starts
// in the output, relative to the tile's first position and cut to 32 bits (0: at or in front of it; past the last document:
// never reached) -- a tile's positions are below kSelTile + kSelChunk, so the cut changes no comparison --, and its delta: where
// the document lies in the text minus where it lies in the output, so that position p of it is text[delta + p].
GFT_HD inline uint32_t sel_window_rel(const uint64_t* c_off, uint64_t m, uint64_t base, uint32_t j, uint64_t tile_lo) {
    if (base + j > m) return 0xFFFFFFFFu;
    const uint64_t v = c_off[base + j];
    return v <= tile_lo ? 0u : (v - tile_lo > 0xFFFFFFFEull ? 0xFFFFFFFEu : (uint32_t)(v - tile_lo));
}
GFT_HD inline uint64_t sel_window_delta(const uint64_t* c_off, const uint64_t* c_src, uint64_t m, uint64_t base, uint32_t j) {
    return base + j < m ? c_src[base + j] - c_off[base + j] : 0;
}
// The largest j with rel(j) <= p_rel, given rel(0) <= p_rel and ascending entries.  rel(j): entry j -- the policy: a shuffle
// across the lanes on the device (every lane of the wave makes every call), an array on the host.  Below kSelWindow - 1 the
// position lies in document base + j and entry j + 1 is where that document ends; kSelWindow - 1: the window does not show it.
template <class At>
GFT_HD inline uint32_t sel_lift(const At& rel, uint32_t p_rel) {
    uint32_t idx = 0;
#pragma unroll
    for (uint32_t s = kSelWindow / 2; s; s >>= 1) {
        const uint32_t v = rel(idx + s);
        if (v <= p_rel) idx += s;
    }
    return idx;
}

// One segment: the part of a document that lies in [p, hi) goes into acc at byte j of the chunk; the document holds p, ends at
// doc_end in the output and has this delta.  Returns where the segment ends.
GFT_HD inline uint64_t sel_segment_at(const uint8_t* text, uint64_t delta, uint64_t doc_end, uint64_t p, uint64_t hi, uint32_t j, SelV& acc) {
    const uint64_t seg_end = doc_end < hi ? doc_end : hi;
    const SelV v = sel_shift(sel_load(text + (delta + p), (uint32_t)(seg_end - p)), j);
    acc.lo |= v.lo; acc.hi |= v.hi;
    return seg_end;
}
// ... of compact document k (c_off[k] <= p < c_off[k + 1]), from the arrays
GFT_HD inline uint64_t sel_segment(const uint8_t* text, const uint64_t* c_off, const uint64_t* c_src, uint64_t k, uint64_t p, uint64_t hi,
                                   uint32_t j, SelV& acc) {
    return sel_segment_at(text, c_src[k] - c_off[k], c_off[k + 1], p, hi, j, acc);
}
// The segments behind the first: the documents after k that meet [p, hi), the empty ones among them stepped over.
GFT_HD inline void sel_more_segments(const uint8_t* text, const uint64_t* c_off, const uint64_t* c_src, uint64_t k, uint64_t p, uint64_t hi,
                                     uint32_t j, SelV& acc) {
    while (p < hi) {
        k++;
        while (c_off[k + 1] <= p) k++;
        const uint64_t q = sel_segment(text, c_off, c_src, k, p, hi, j, acc);
        j += (uint32_t)(q - p);
        p = q;
    }
}
// chunk c's positions [lo, hi) from acc: one 16-byte store to an address that is a multiple of 16 when all sixteen are in range,
// bytes otherwise
GFT_HD inline void sel_store(uint8_t* out, const SelGeom& G, uint64_t c, uint64_t lo, uint64_t hi, const SelV& acc) {
    if (hi - lo == kSelChunk) {
#if defined(__HIP_DEVICE_COMPILE__)
        struct __attribute__((aligned(16))) U128a { uint64_t lo, hi; };
        *reinterpret_cast<U128a*>(out + lo) = U128a{acc.lo, acc.hi};
#else
        uint8_t b[16];
        for (uint32_t i = 0; i < 8; i++) { b[i] = (uint8_t)(acc.lo >> (8 * i)); b[8 + i] = (uint8_t)(acc.hi >> (8 * i)); }
        memcpy(out + lo, b, 16);
#endif
        return;
    }
    for (uint64_t p = lo; p < hi; p++) {
        const uint32_t j = sel_chunk_byte(G, c, p);
        out[p] = (uint8_t)((j < 8 ? acc.lo >> (8 * j) : acc.hi >> (8 * (j - 8))) & 0xFFu);
    }
}

}  // namespace gft
