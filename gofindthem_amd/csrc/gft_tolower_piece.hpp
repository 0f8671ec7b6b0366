// gft_tolower_piece.hpp -- strings.ToLower (finder/finder.go:140-142) over one 16-byte piece of a document, compiled for the
// host and for the device: the kernels of gft_tolower.hip and the host walk of tolower_host.cpp (gft_debug_emulate_to_lower)
// run this one source.
//
// Go's decoder, data-parallel.  A lead byte is never a continuation byte, so every byte that is not a continuation byte
// starts a rune: a valid sequence of 2..4 bytes, or -- anything else -- one U+FFFD that advances one byte.  A continuation
// byte belongs to a rune exactly when one of the three bytes in front of it is a lead byte whose whole, valid sequence
// reaches it; otherwise it is one U+FFFD of its own.  Documents are judged one by one: bytes outside the document are read
// as 0x00 here, which is neither a lead nor a continuation byte -- a lead byte at a document's end stays unfinished, a
// continuation byte at a document's start has no lead.  So the output of a piece depends on its own bytes, three bytes in
// front of them and three behind them.
//
// A piece holds n <= 16 bytes of its unit; the window around it is 3 + 16 + 4 bytes in six dwords (tolower_load_piece).  All
// loops below have constant trip counts and unroll completely: the window stays in registers.
// Needs GFT_HD (gft_kernels.hpp).
#pragma once
#include <stdint.h>

namespace gft {

constexpr uint32_t kLowerPiece = 16;             // bytes per lane
constexpr uint32_t kLowerChunk = 64 * kLowerPiece;   // bytes per wave and trip
constexpr uint32_t kLowerUnitMax = 8192;         // bytes per work unit {doc, lo, hi}: eight trips
constexpr uint32_t kLowerPageShift = 6;          // code points per page of the mapping table: 64

// The mapping, two levels: page[cp >> 6] = 0 (no code point of the page has another lower-case form) or the page's row of
// `delta`; delta[row * 64 + (cp & 63)] = lower(cp) - cp.  Pages at and above n_pages are identity.  Derived from the pairs
// of unicode_lower.inc when an engine is created (tolower_host.cpp); ASCII is folded arithmetically.
struct LowerTable {
    const uint16_t* page;
    const int32_t* delta;
    uint32_t n_pages;
};

GFT_HD inline uint32_t tolower_rune(const LowerTable& T, uint32_t cp) {
    if (cp < 0x80u) return cp + ((cp - 'A') < 26u ? 32u : 0u);
    const uint32_t pg = cp >> kLowerPageShift;
    if (pg >= T.n_pages) return cp;
    const uint32_t row = T.page[pg];
    return row ? cp + (uint32_t)T.delta[row * 64u + (cp & 63u)] : cp;
}

struct __attribute__((packed, aligned(1))) LowerU32u { uint32_t v; };
struct __attribute__((packed, aligned(1))) LowerU128u { uint32_t x, y, z, w; };

// window of a piece: d[0] = the three bytes in front (byte -1 in bits 24..31), d[1..4] = the piece, d[5] = the bytes behind
struct LowerWin { uint32_t d[6]; };

// byte j of the window, -3 <= j <= 19 (j is a constant wherever this is called)
GFT_HD inline uint32_t tolower_win_byte(const LowerWin& w, int j) { return (w.d[(j + 4) >> 2] >> (8 * ((j + 4) & 3))) & 0xFFu; }

// Loads the window of the piece at p.  back = bytes of the document in front of the piece, at most 3; avail = bytes of the
// document from the piece's first byte on (>= 1: the own bytes and what follows them, whatever unit it belongs to).  Bytes
// outside the document become 0x00.  Reads p[-back .. 19]: the blob is readable 64 bytes past its end (gft.h).
GFT_HD inline void tolower_load_piece(const uint8_t* p, uint32_t back, uint64_t avail, LowerWin& w) {
    const LowerU128u v = *reinterpret_cast<const LowerU128u*>(p);
    uint32_t prev = 0;
    if (back >= 1) prev |= (uint32_t)p[-1] << 24;
    if (back >= 2) prev |= (uint32_t)p[-2] << 16;
    if (back >= 3) prev |= (uint32_t)p[-3] << 8;
    w.d[0] = prev; w.d[1] = v.x; w.d[2] = v.y; w.d[3] = v.z; w.d[4] = v.w;
    w.d[5] = reinterpret_cast<const LowerU32u*>(p + 16)->v;
    const uint32_t hi = avail < 20 ? (uint32_t)avail : 20u;
#pragma unroll
    for (uint32_t q = 0; q < 5; q++) {
        const uint32_t keep = hi > 4 * q ? hi - 4 * q : 0u;
        w.d[q + 1] &= keep >= 4 ? 0xFFFFFFFFu : (1u << (8 * keep)) - 1u;
    }
}

// the n own bytes hold no byte >= 0x80: the piece is its own A-Z fold
GFT_HD inline bool tolower_piece_ascii(const LowerWin& w, uint32_t n) {
    uint32_t acc = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) {
        const uint32_t keep = n > 4 * q ? n - 4 * q : 0u;
        acc |= w.d[q + 1] & (keep >= 4 ? 0xFFFFFFFFu : (1u << (8 * keep)) - 1u);
    }
    return (acc & 0x80808080u) == 0;
}

// ASCII lower-casing of four packed bytes, none of them >= 0x80
GFT_HD inline uint32_t tolower_fold4(uint32_t w) {
    const uint32_t ge_a = w + 0x3F3F3F3Fu;          // bit 7 set where byte >= 'A'
    const uint32_t gt_z = w + 0x25252525u;          // bit 7 set where byte >  'Z'
    return w | ((ge_a & ~gt_z & 0x80808080u) >> 2);
}

// Go's utf8.DecodeRune on the bytes b0 b1 b2 b3 (0x00 where the document has none): length of the valid sequence that b0
// leads and its code point, or 0 -- b0 is then one U+FFFD (C0 / C1 / F5..FF, overlong E0 80..9F / F0 80..8F, surrogates
// ED A0..BF, F4 90.., a sequence cut short).  b0 >= 0xC0.
GFT_HD inline uint32_t tolower_decode(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3, uint32_t& cp) {
    const bool c2 = (b2 & 0xC0u) == 0x80u, c3 = (b3 & 0xC0u) == 0x80u;
    if (b0 < 0xE0u) {
        cp = (b0 & 0x1Fu) << 6 | (b1 & 0x3Fu);
        return b0 >= 0xC2u && (b1 & 0xC0u) == 0x80u ? 2u : 0u;
    }
    if (b0 < 0xF0u) {
        const uint32_t lo = b0 == 0xE0u ? 0xA0u : 0x80u, hi = b0 == 0xEDu ? 0x9Fu : 0xBFu;
        cp = (b0 & 0x0Fu) << 12 | (b1 & 0x3Fu) << 6 | (b2 & 0x3Fu);
        return b1 >= lo && b1 <= hi && c2 ? 3u : 0u;
    }
    const uint32_t lo = b0 == 0xF0u ? 0x90u : 0x80u, hi = b0 == 0xF4u ? 0x8Fu : 0xBFu;
    cp = (b0 & 0x07u) << 18 | (b1 & 0x3Fu) << 12 | (b2 & 0x3Fu) << 6 | (b3 & 0x3Fu);
    return b0 <= 0xF4u && b1 >= lo && b1 <= hi && c2 && c3 ? 4u : 0u;
}

// UTF-8 of cp (a valid scalar value), first byte in bits 0..7; returns its length
GFT_HD inline uint32_t tolower_encode(uint32_t cp, uint32_t& bytes) {
    if (cp < 0x80u) { bytes = cp; return 1; }
    if (cp < 0x800u) { bytes = (0xC0u | cp >> 6) | (0x80u | (cp & 0x3Fu)) << 8; return 2; }
    if (cp < 0x10000u) { bytes = (0xE0u | cp >> 12) | (0x80u | (cp >> 6 & 0x3Fu)) << 8 | (0x80u | (cp & 0x3Fu)) << 16; return 3; }
    bytes = (0xF0u | cp >> 18) | (0x80u | (cp >> 12 & 0x3Fu)) << 8 | (0x80u | (cp >> 6 & 0x3Fu)) << 16 | (0x80u | (cp & 0x3Fu)) << 24;
    return 4;
}

// the output stream of a piece: bytes gather in a 64-bit register and leave as dwords; nothing is stored at or past cap
struct LowerEmit {
    uint8_t* out;
    uint64_t pos, cap;
    uint64_t acc;
    uint32_t fill;
};
GFT_HD inline void tolower_store4(uint8_t* out, uint64_t pos, uint64_t cap, uint32_t v) {
    if (pos + 4 <= cap) {
        reinterpret_cast<LowerU32u*>(out + pos)->v = v;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 4; k++)
            if (pos + k < cap) out[pos + k] = (uint8_t)(v >> (8 * k));
    }
}
template <bool WRITE>
GFT_HD inline void tolower_emit(LowerEmit& e, uint32_t bytes, uint32_t len) {
    if (!WRITE) return;
    e.acc |= (uint64_t)bytes << (8 * e.fill);
    e.fill += len;
    if (e.fill >= 4) {
        tolower_store4(e.out, e.pos, e.cap, (uint32_t)e.acc);
        e.acc >>= 32; e.fill -= 4; e.pos += 4;
    }
}
GFT_HD inline void tolower_flush(LowerEmit& e) {
#pragma unroll
    for (uint32_t k = 0; k < 3; k++)
        if (k < e.fill && e.pos + k < e.cap) e.out[e.pos + k] = (uint8_t)(e.acc >> (8 * k));
}

// The lower-case form of the piece's n own bytes: returns its length; WRITE: stores it at out[pos ..), below cap only.
template <bool WRITE>
GFT_HD inline uint32_t tolower_piece(const LowerTable& T, const LowerWin& w, uint32_t n, uint8_t* out, uint64_t pos, uint64_t cap) {
    if (tolower_piece_ascii(w, n)) {
        if (WRITE) {
            if (n == kLowerPiece && pos + kLowerPiece <= cap) {
                LowerU128u v;
                v.x = tolower_fold4(w.d[1]); v.y = tolower_fold4(w.d[2]); v.z = tolower_fold4(w.d[3]); v.w = tolower_fold4(w.d[4]);
                *reinterpret_cast<LowerU128u*>(out + pos) = v;
            } else {
#pragma unroll
                for (uint32_t q = 0; q < 4; q++)
                    if (n > 4 * q) tolower_store4(out, pos + 4 * q, pos + n < cap ? pos + n : cap, tolower_fold4(w.d[q + 1]));
            }
        }
        return n;
    }
    LowerEmit e{out, pos, cap, 0, 0};
    uint32_t total = 0;
    uint32_t covered = 0;                           // bit j + 3: byte j belongs to the rune of a lead byte in front of it
#pragma unroll
    for (int j = -3; j < (int)kLowerPiece; j++) {
        const uint32_t b = tolower_win_byte(w, j);
        const bool own = j >= 0 && (uint32_t)j < n;
        uint32_t bytes = 0xBDBFEFu, len = 3;        // U+FFFD
        if (b >= 0xC0u) {
            uint32_t cp;
            const uint32_t L = tolower_decode(b, tolower_win_byte(w, j + 1), tolower_win_byte(w, j + 2), tolower_win_byte(w, j + 3), cp);
            if (L) {
                covered |= ((1u << (L - 1)) - 1u) << (j + 4);
                if (own) len = tolower_encode(tolower_rune(T, cp), bytes);
            }
        } else if (b >= 0x80u) {
            if (covered >> (j + 3) & 1u) len = 0;
        } else {
            bytes = b + ((b - 'A') < 26u ? 32u : 0u);
            len = 1;
        }
        if (own) {
            total += len;
            if (len) tolower_emit<WRITE>(e, bytes, len);
        }
    }
    if (WRITE) tolower_flush(e);
    return total;
}

// The rune of the piece whose lower-case form holds byte t of the piece's output (t < tolower_piece<false>'s figure): returns
// the index of its first byte among the piece's own bytes, src_len = the source bytes it takes -- 1 for an ASCII or an invalid
// byte, 2..4 for a valid sequence, which may reach past the piece's end.  The walk of tolower_piece, without the stores: a
// continuation byte that a lead in front of it covers has no output and is never the answer.  kLowerPiece when t is not below
// the piece's output length.
GFT_HD inline uint32_t tolower_piece_rune_at(const LowerTable& T, const LowerWin& w, uint32_t n, uint32_t t, uint32_t& src_len) {
    src_len = 1;
    if (tolower_piece_ascii(w, n)) return t < n ? t : kLowerPiece;
    uint32_t total = 0, at = kLowerPiece;
    uint32_t covered = 0;
#pragma unroll
    for (int j = -3; j < (int)kLowerPiece; j++) {
        const uint32_t b = tolower_win_byte(w, j);
        const bool own = j >= 0 && (uint32_t)j < n;
        uint32_t bytes, len = 3, sl = 1;            // U+FFFD from one byte
        if (b >= 0xC0u) {
            uint32_t cp;
            const uint32_t L = tolower_decode(b, tolower_win_byte(w, j + 1), tolower_win_byte(w, j + 2), tolower_win_byte(w, j + 3), cp);
            if (L) {
                covered |= ((1u << (L - 1)) - 1u) << (j + 4);
                sl = L;
                if (own) len = tolower_encode(tolower_rune(T, cp), bytes);
            }
        } else if (b >= 0x80u) {
            if (covered >> (j + 3) & 1u) len = 0;
        } else {
            len = 1;
        }
        if (own) {
            if (at == kLowerPiece && t - total < len) { at = (uint32_t)j; src_len = sl; }   // (t >= total while at is unset)
            total += len;
        }
    }
    return at;
}

}  // namespace gft
